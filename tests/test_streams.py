"""Every stream-taking call on a stream that is not the default one (include/wedm_hip.h: "launches are asynchronous on the
`hipStream_t` passed as `void* stream`").

On the legacy default stream a launch that dropped its stream argument, a wrapper that picked another stream and a hidden
synchronisation all leave every result as it was: the default stream orders itself against everything.  Here each of the
nine entry points -- `wedm_step`, `wedm_reset`, `wedm_copy_columns`, `wedm_wire_profile`, `wedm_derive_geometry`,
`wedm_draw_episode`, `wedm_normalize`, `wedm_gae`, `wedm_policy_head` -- runs on a side stream behind a gate
(tests/_stream_gate.py): the inputs hold valid values A, the side stream gets the gate, copies of valid values B into the same
buffers and the call, and a control -- the same call on the same input buffers, into outputs of its own -- goes out on the
default stream.  After one synchronise

  1. everything the call wrote is B's definition on every byte, its inputs hold B, guard bands are intact;
  2. the control's outputs are A's definition and not B's (so the gate held, in this run, on this machine), and A's and B's
     definitions differ in every block the call writes (asserted on the host before anything is launched);
  3. the event recorded behind the call had not happened when the call returned, and has happened after the synchronise.

Where a call's main input alone cannot change a block (a GAE's ``valid`` row follows the done flags, not the rewards; a
normaliser's episode rows follow the rewards and done flags, not the observations), the flags and rewards are gated with it,
so that 2 holds for every block.  `wedm_step` latches its action at control steps only, 1000 us apart: the environments
start with ``time_since_servo`` at the control interval, so the launch of 1 us latches the action it is given, and with the
progress reward, so the reward block differs too.

Then two handles on two side streams at once, a handle handed from one stream to another through an event, and the whole
stack -- vector adapter, normaliser, policy head, rollout buffer -- running ahead of the host on a side stream.  No graph is
captured anywhere: `wedm_step` picks its instantiation and its trace slot on the host when it is enqueued."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from sparc_amd import (Normalizer, PolicyHead, RolloutBuffer, WireEDMEnv, WireEDMVectorEnv, WireModuleParameters, _abi)
from sparc_amd.normalize import ROW_NAMES, STEP, UPDATE
from sparc_amd.policy_head import BACKWARD, EVALUATE, SAMPLE
from sparc_amd.rollout import NORMALIZE, SCAN_UNROLL, SKIP_AFTER_DONE
from tests import _episode_draw_ref as draw_ref
from tests import _geometry_ref as geom_ref
from tests import _registry_catalogue as cat
from tests import test_episode_sampler as sampler
from tests import test_geometry as geometry
from tests import test_normalize as norm
from tests import test_policy_head as head
from tests import test_registry_coverage as cov
from tests import test_rollout as rollout
from tests import test_snapshot as snap
from tests import test_wire_profile as profile
from tests._compare import block_diffs
from tests._normalize_common import columns, same_bits
from tests._policy_head_common import random_params
from tests._signal_oracle import SignalOracleBackend
from tests._snapshot_common import assert_same, copy_columns_numpy, diffs, everything, make, scenario
from tests._stream_gate import DEV, Gate, check_control, gated, seconds_on
from tests._wire_profile_ref import pack, reference_rows

pytestmark = pytest.mark.gpu

N_ENVS, N_SEG = 100, 99                       # tests/test_registry_coverage.py: every family's last block is partly dead
ACTION = {"A": (0.1, 80.0, 17, 3.0, 20.0), "B": (0.05, 80.0, 13, 2.0, 20.0)}
LEAVES = ("servo", "target_voltage", "on_time", "off_time", "current_mode")
LAUNCHES = (1, 290)
# (id, kernel, lanes, trace bound): the automatic plan, the two-lane register kernel, kernel 1 with a sample in the launch
STEP_CASES = (("auto", 0, 0, False), ("regs2", 7, 2, False), ("global-traced", 1, 0, True))


def _bytes_differ(a, b) -> bool:
    return not same_bits(a, b)


# ------------------------------------------------------------------------------------------------ wedm_step: the harness
def _step_env(device):
    """The environment of tests/test_registry_coverage.py (100 x 99, no binding) with the progress reward.  The twin runs on
    `SignalOracleBackend`, which forms a launch's reward over the whole launch (the plain seam runs a traced launch as
    pieces between samples, and would leave the last piece's reward)."""
    kw = dict(cov._kw(N_SEG, N_ENVS, frozenset(), False), reward="progress")
    if device == "cpu":
        kw["backend"] = SignalOracleBackend
    env = WireEDMEnv(num_envs=N_ENVS, device=device, **kw)
    assert env.n_segments == N_SEG
    return env


def _step_start(env):
    """That test's scenario, with the first step a control step: the launch of 1 us latches the action it reads."""
    act = cov._scenario(env, N_SEG)
    env.state.time_since_servo = env.servo_interval
    return act


def _bind(env, traced):
    return env.bind_trace(cat.TRACE_SIGNALS, every=cat.TRACE_EVERY, capacity=cat.TRACE_CAPACITY) if traced else None


@functools.lru_cache(maxsize=None)
def _step_reference(which, traced):
    """The oracle's (blocks, trace ring, sample count) after the launches with action A or B: computed once, left unchanged."""
    env = _step_env("cpu")
    _step_start(env)
    act = env.make_action(*ACTION[which])
    trace = _bind(env, traced)
    for us in LAUNCHES:
        env.step_many(act, us)
    assert bool(env.state.is_wire_broken[5]) and int(env.state.spark_count.sum()) > 0 and not bool(env.state.error.any())
    return cov._snapshot(env, trace)


def _step_matches(got, want) -> bool:
    (blocks, ring, count), (w_blocks, w_ring, w_count) = got, want
    if block_diffs(blocks, w_blocks, N_ENVS) or count != w_count:
        return False
    return w_ring is None or all(cov._same(ring[name], w_ring[name]) for name in cat.TRACE_SIGNALS)


def _slowest_call() -> float:
    """Seconds of the slowest call under test alone on the default stream, after a warm-up: the launches of every `wedm_step`
    case, and a control step of the whole stack (a launch of 1000 us)."""
    slowest = 0.0
    for _, kernel, lanes, traced in STEP_CASES:
        env = _step_env(DEV)
        env.set_kernel(kernel, lanes)
        act = _step_start(env)
        _bind(env, traced)

        def launches():
            for us in LAUNCHES:
                env.step_many(act, us)

        launches()   # warm-up: plans made, code loaded
        slowest = max(slowest, seconds_on(torch.cuda.default_stream(), launches))
        env.close()
    vec, run = _stack()
    run()
    slowest = max(slowest, seconds_on(torch.cuda.default_stream(), run) / STACK_T)
    vec.close()
    return slowest


@pytest.fixture(scope="module")
def gate():
    g = Gate(_slowest_call())
    print(f"\n[streams] {g}")
    return g


# ------------------------------------------------------------------------------------------------ 1. the stream lookup
def test_the_backend_hands_the_library_torchs_current_stream():
    env = make(DEV, 4)
    be, S = env._backend, torch.cuda.Stream(device=DEV)
    default = torch.cuda.default_stream(DEV).cuda_stream
    raw = be._raw_stream
    assert raw is not None, "this torch build has the raw accessor"
    assert S.cuda_stream != default
    try:
        for accessor in (raw, None):   # the raw accessor, then the fallback through torch.cuda.current_stream
            be._raw_stream = accessor
            assert (be._stream().value or 0) == default
            with torch.cuda.stream(S):
                assert be._stream().value == S.cuda_stream
            assert (be._stream().value or 0) == default
    finally:
        be._raw_stream = raw
        env.close()


# ------------------------------------------------------------------------------------------------ 2. wedm_step
@pytest.mark.parametrize("kernel,lanes,traced", [c[1:] for c in STEP_CASES], ids=[c[0] for c in STEP_CASES])
def test_step_behind_the_gate(gate, kernel, lanes, traced):
    """100 x 99, the scenario of tests/test_registry_coverage.py, launches of 1 and 290 us with nothing between them; the five
    action leaves are the gated input.  (The host runs ahead of the device here, so the launch of 290 us is planned before
    any kernel has reported environment 5's broken wire: the instantiation without frozen-lane code meets a frozen lane.)"""
    want_a, want_b = _step_reference("A", traced), _step_reference("B", traced)
    same = [k for k in want_a[0] if not _bytes_differ(want_a[0][k], want_b[0][k])]
    assert not same, f"A's and B's definitions agree in {same}"
    if traced:
        assert want_a[2] == want_b[2] == sum(LAUNCHES) // cat.TRACE_EVERY
        assert all(_bytes_differ(want_a[1][name], want_b[1][name]) for name in cat.TRACE_SIGNALS)
    gpu, ctl = _step_env(DEV), _step_env(DEV)
    try:
        for env in (gpu, ctl):
            env.set_kernel(kernel, lanes)
        act = _step_start(gpu)
        _step_start(ctl)
        b = gpu.make_action(*ACTION["B"])
        trace_g, trace_c = _bind(gpu, traced), _bind(ctl, traced)

        def write_b():
            for name in LEAVES:
                getattr(act, name).copy_(getattr(b, name))

        def launches(env):
            def go():
                for us in LAUNCHES:
                    env.step_many(act, us)
            return go

        gated(gate, write_b, launches(gpu), launches(ctl))
        name = gpu._backend.last_kernel()
        assert kernel == 0 or ("wedm_step_regs<2>" if kernel == 7 else "wedm_step_global") in name, name
        assert all(torch.equal(getattr(act, leaf), getattr(b, leaf)) for leaf in LEAVES), "an action leaf was written"
        cov._compare(gpu, trace_g, want_b, N_ENVS, f"wedm_step behind the gate ({name})")
        got = cov._snapshot(ctl, trace_c)
        check_control(_step_matches(got, want_a), _step_matches(got, want_b), gate, "wedm_step")
    finally:
        gpu.close()
        ctl.close()


# ------------------------------------------------------------------------------------------------ 3. wedm_reset
def test_reset_behind_the_gate(gate):
    """100 environments with every binding (pulse and signal statistics among them: all three reset kernels run), stepped
    through a control step and 300 us of sparks; the device mask is the gated input: A the even environments, B the odd."""
    n = N_ENVS

    def start(env):
        act = scenario(env)
        env.state.time_since_servo = env.servo_interval   # a control step: the observation rows are written
        env.step_many(act, 300)

    cpu = make("cpu", n, "all", "s13")
    start(cpu)
    before = everything(cpu)
    saved = cpu.state.clone_blocks()
    masks = {"A": np.arange(n) % 2 == 0, "B": np.arange(n) % 2 == 1}
    want = {}
    for which, m in masks.items():
        cpu.state.load_blocks(saved)
        cpu.reset(options={"mask": torch.from_numpy(m)})
        want[which] = everything(cpu)
    written = sorted(k for k in before if any(_bytes_differ(before[k], want[w][k]) for w in "AB"))
    assert {"f64", "i32", "i8", "T", "obs", "pulse", "signal"} <= set(written), written
    assert all(_bytes_differ(want["A"][k], want["B"][k]) for k in written)
    gpu, ctl = make(DEV, n, "all", "s13"), make(DEV, n, "all", "s13")
    try:
        for env in (gpu, ctl):
            start(env)
        torch.cuda.synchronize()
        assert_same(everything(gpu), before, "the start")
        mask = torch.from_numpy(masks["A"].astype(np.uint8)).to(DEV)
        mask_b = torch.from_numpy(masks["B"].astype(np.uint8)).to(DEV)
        gated(gate, lambda: mask.copy_(mask_b), lambda: gpu.reset(options={"mask": mask}),
              lambda: ctl.reset(options={"mask": mask}))
        assert gpu._mask_buf.data_ptr() == mask.data_ptr(), "the launch read the gated buffer itself"
        assert torch.equal(mask, mask_b)
        assert_same(everything(gpu), want["B"], "wedm_reset behind the gate")
        got = everything(ctl)
        check_control(not diffs(got, want["A"]), not diffs(got, want["B"]), gate, "wedm_reset")
    finally:
        gpu.close()
        ctl.close()


# ------------------------------------------------------------------------------------------------ 4. wedm_copy_columns
def test_copy_columns_behind_the_gate(gate):
    """A fork in place on four planes (every element width, partial and full items) of 600 columns: 257 pairs -- a block of
    256 and a block with one live lane -- from the first 300 columns into the last 300; the two index lists are the gated
    input."""
    env, be = snap._backend()
    gen, rng = torch.Generator(device=DEV).manual_seed(7), np.random.default_rng(7)
    shapes, cols, stride, count = ((1, 7), (4, 9), (8, 8), (16, 33)), 600, 640, 257
    planes = [snap.Plane(gen, r, stride, w) for w, r in shapes]
    twins = [snap.Plane(gen, r, stride, w) for w, r in shapes]
    for p, t in zip(planes, twins):
        t.raw.copy_(p.raw)
    lists = {w: (rng.integers(0, 300, count), 300 + rng.permutation(300)[:count]) for w in "AB"}
    start = {f"plane{k}": p.tensor.cpu() for k, p in enumerate(planes)}
    want = {w: copy_columns_numpy(start, s.tolist(), d.tolist()) for w, (s, d) in lists.items()}
    assert all(_bytes_differ(want["A"][k], want["B"][k]) for k in start)
    si, di = snap._dev(lists["A"][0]), snap._dev(lists["A"][1])
    si_b, di_b = snap._dev(lists["B"][0]), snap._dev(lists["B"][1])
    status, status_c = (torch.zeros(1, dtype=torch.int32, device=DEV) for _ in range(2))
    warm = snap.Plane(gen, 9, stride, 4)
    be.copy_columns([snap._cplane(warm, warm, cols, cols)], si.data_ptr(), di.data_ptr(), count, None)   # warm-up

    def write_b():
        si.copy_(si_b)
        di.copy_(di_b)

    def call(ps, st):
        return lambda: be.copy_columns([snap._cplane(p, p, cols, cols) for p in ps], si.data_ptr(), di.data_ptr(), count,
                                       st.data_ptr())

    gated(gate, write_b, call(planes, status), call(twins, status_c))
    assert torch.equal(si, si_b) and torch.equal(di, di_b) and int(status.item()) == 0 and int(status_c.item()) == 0
    for k, (p, t) in enumerate(zip(planes, twins)):
        assert same_bits(p.tensor, want["B"][f"plane{k}"]), f"wedm_copy_columns behind the gate: plane {k}"
        for q in (p, t):
            assert bool((q.raw[: q.band] == snap.FILL).all()) and bool((q.raw[-q.band:] == snap.FILL).all())
    check_control(all(same_bits(t.tensor, want["A"][f"plane{k}"]) for k, t in enumerate(twins)),
                  any(same_bits(t.tensor, want["B"][f"plane{k}"]) for k, t in enumerate(twins)), gate, "wedm_copy_columns")
    env.close()


# ------------------------------------------------------------------------------------------------ 5. wedm_wire_profile
def test_wire_profile_behind_the_gate(gate):
    """70 environments of up to 5 cells at stride 75, per-environment lengths and zones, 3 bins; the wire block is the gated
    input."""
    num_envs, n_max, stride, out_stride = 70, 5, 75, 70
    bins, dead = 3, np.float32(1.0e30)
    rng = np.random.default_rng(70)
    env = make(DEV, 4)
    cells = {w: rng.uniform(250.0, 4000.0, (num_envs, n_max)).astype(np.float32) for w in "AB"}
    n, zs, ze = profile._geometry(rng, num_envs, n_max, True)
    want = {w: reference_rows(c, n, zs, ze, bins) for w, c in cells.items()}
    assert all((want["A"][r] != want["B"][r]).any() for r in range(want["A"].shape[0]))
    call = profile.Call(env._backend, cells["A"], n, zs, ze, stride, True, dead, out_stride)
    T_b = torch.from_numpy(pack(cells["B"], n, stride, dead)).to(DEV)
    geom = call.geom.clone()
    outs = [torch.full((_abi.profile_rows(bins), out_stride), float(profile.SENTINEL), dtype=torch.float32, device=DEV)
            for _ in range(3)]
    call.run(bins, out=outs[2])   # warm-up
    gated(gate, lambda: call.T.copy_(T_b), lambda: call.run(bins, out=outs[0], sync=False),
          lambda: call.run(bins, out=outs[1], sync=False))
    assert torch.equal(call.T.view(torch.int32), T_b.view(torch.int32)) and torch.equal(call.geom, geom)
    assert int(call.status.item()) == 0
    got, control = outs[0].cpu().numpy(), outs[1].cpu().numpy()
    assert profile.same_bits(got, want["B"]), "wedm_wire_profile behind the gate"
    check_control(profile.same_bits(control, want["A"]), profile.same_bits(control, want["B"]), gate, "wedm_wire_profile")
    env.close()


# ------------------------------------------------------------------------------------------------ 6. wedm_derive_geometry
def test_derive_geometry_behind_the_gate(gate):
    """100 environments at stride 128, two materials by three diameters, a scattered mask, canaries around and between; the
    heights are the gated input."""
    n, stride, n_max = N_ENVS, 128, 70
    combo = geom_ref.combination_table([geom_ref.BRASS, geom_ref.COPPER], geometry.DIAMETERS, geometry.WIRE, geometry.MP)
    heights = {"A": np.linspace(1.0, 10.0, n), "B": np.linspace(9.5, 1.5, n)}
    di, mi, mask = np.arange(n) % 3, (np.arange(n) // 3) % 2, np.arange(n) % 5 != 2
    call = geometry.DeriveCall(geometry.WIRE, combo, 3, n_max, stride, heights["A"], di, mi, mask)
    h_b = torch.from_numpy(heights["B"]).to(DEV)
    blocks = {w: call.blocks() for w in ("A", "B", "warm")}
    want = {}
    for w in "AB":
        host_f, host_i = blocks[w][:2]
        status = geom_ref.derive_columns(host_f[1:-1], host_i[1:-1], geometry.WIRE, combo, 3, n_max, heights[w], di, mi, mask)
        want[w] = (host_f, host_i, status)
    assert want["A"][0].tobytes() != want["B"][0].tobytes() and want["A"][1].tobytes() != want["B"][1].tobytes()
    call.launch(*blocks["warm"][2:])   # warm-up
    gated(gate, lambda: call.height.copy_(h_b), lambda: call.launch(*blocks["B"][2:]), lambda: call.launch(*blocks["A"][2:]))
    assert torch.equal(call.height, h_b)
    got = {w: (blocks[w][2].cpu().numpy(), blocks[w][3].cpu().numpy(), int(blocks[w][4].item())) for w in "AB"}
    geometry.assert_same(got["B"], want["B"])   # guard rows, padding and unmasked columns included
    assert got["B"][2] == 0

    def equal(a, b):
        return a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and a[2] == b[2]

    check_control(equal(got["A"], want["A"]), equal(got["A"], want["B"]), gate, "wedm_derive_geometry")


# ------------------------------------------------------------------------------------------------ 7. wedm_draw_episode
def test_draw_episode_behind_the_gate(gate):
    """257 environments at stride 320, every slot drawn, dynamic geometry; the mask is the gated input: A the even
    environments, B the odd.  The call works in place, so the control draws on a twin set of blocks in the same state."""
    n, stride, case = 257, 320, sampler.CASES[5]
    masks = {"A": np.arange(n) % 2 == 0, "B": np.arange(n) % 2 == 1}
    sets = {w: sampler.setup_call(n, stride, None, case) for w in ("A", "B", "warm")}
    want = {}
    for w in "AB":
        alloc, tables, _, _, _, _, spec, geom, _ = sets[w]
        b = draw_ref.inner(alloc)
        b.update(tables)
        assert draw_ref.draw_columns(b, spec, sampler.SEED, 0, n, masks[w], sampler.CONSTS, geom) == 0
        want[w] = alloc
    assert all(want["A"][name].tobytes() != want["B"][name].tobytes() for name in want["A"])
    mask = torch.from_numpy(masks["A"].astype(np.uint8)).to(DEV)
    mask_b = torch.from_numpy(masks["B"].astype(np.uint8)).to(DEV)

    def call(w):
        def go():
            rc, text = sampler.launch(sets[w][5], mask, sets[w][4]["count"])
            assert rc == _abi.OK, text
        return go

    call("warm")()   # warm-up
    gated(gate, lambda: mask.copy_(mask_b), call("B"), call("A"))
    assert torch.equal(mask, mask_b)
    got = {w: {name: t.cpu().numpy() for name, t in sets[w][2].items()} for w in "AB"}
    for name, a in want["B"].items():   # whole allocations: guard rows, padding columns and unmasked columns
        assert got["B"][name].tobytes() == a.tobytes(), f"wedm_draw_episode behind the gate: {name}"
    for w in "AB":
        assert int(sets[w][3]["status"].item()) == 0
        for name, t in sets[w][1].items():
            assert sets[w][3][name].cpu().numpy().tobytes() == t.tobytes(), name
    check_control(all(got["A"][name].tobytes() == a.tobytes() for name, a in want["A"].items()),
                  any(got["A"][name].tobytes() == a.tobytes() for name, a in want["B"].items()), gate, "wedm_draw_episode")


# ------------------------------------------------------------------------------------------------ 8. wedm_normalize
def _norm_differences(dev, host):
    """`Problem.differences` of tests/test_normalize.py with the device's and the host's side from two problems."""
    pairs = dict(stats_out=(dev.stats[dev.cur].t, host.stats_h), partials=(dev.partials.t, host.partials_h),
                 obs_out=(dev.obs_out.t, host.obs_h), reward_out=(dev.reward_out.t, host.reward_out_h))
    pairs.update({name: (dev.rows[name].t, host.rows_h[name]) for name in ROW_NAMES})
    return [name for name, (got, want) in pairs.items() if not same_bits(got, want)]


def test_normalize_behind_the_gate(gate):
    """257 environments (two tiles, the second with one live lane) by 9 columns over two planes, mask and skip given, one
    call that reduces, folds and applies.  The observation planes are the gated input, and with them the reward and the two
    done flags (the reward output and the episode rows follow those alone).  The control is a twin problem in the same
    state that reads the same input buffers."""
    flags, N, D = UPDATE | STEP, 257, 9
    p, q = (norm.Problem(N, D, seed=8, split=3) for _ in range(2))
    norm.Problem(N, D, seed=9, split=3).call(flags)   # warm-up
    q.planes, q.reward, q.term, q.trunc = p.planes, p.reward, p.term, p.trunc
    rng = np.random.default_rng(88)
    x, lo = columns(rng, N, D), 0
    planes_b = []
    for a in p.planes_h:
        block = np.full(a.shape, np.nan, dtype=np.float32)
        block[:, :N] = x[lo: lo + a.shape[0]]
        planes_b.append(block)
        lo += a.shape[0]
    reward_b, term_b, trunc_b = rng.normal(size=N).astype(np.float32), rng.random(N) < 0.3, rng.random(N) < 0.3
    dev_b = [torch.from_numpy(a).to(DEV) for a in planes_b + [reward_b, term_b, trunc_b]]
    p.planes_h, p.reward_h, p.term_h, p.trunc_h = planes_b, reward_b, term_b, trunc_b
    before = {name: b.t.clone() for name, b in p.inputs().items() if name in ("mask", "skip", "stats_in")}
    blocks = {**p.blocks(), **{f"twin {k}": v for k, v in q.blocks().items()}}
    p.expect(flags)
    q.expect(flags)
    names = ("stats_h", "partials_h", "obs_h", "reward_out_h")
    same = [k for k in names if not _bytes_differ(getattr(p, k), getattr(q, k))]
    same += [k for k in ROW_NAMES if not _bytes_differ(p.rows_h[k], q.rows_h[k])]
    assert not same, f"A's and B's definitions agree in {same}"

    def write_b():
        for banded, t in zip(p.planes + [p.reward, p.term, p.trunc], dev_b):
            banded.t.copy_(t)

    gated(gate, write_b, lambda: p.call(flags), lambda: q.call(flags))
    p.flip()
    q.flip()
    assert _norm_differences(p, p) == [], "wedm_normalize behind the gate"
    assert all(same_bits(b.t, t) for b, t in zip(p.planes + [p.reward, p.term, p.trunc], dev_b)), "an input was written"
    assert all(same_bits(blocks[name].t, t) for name, t in before.items()), "an input was written"
    assert [name for name, b in blocks.items() if not b.bands_intact()] == []
    check_control(_norm_differences(q, q) == [], len(_norm_differences(q, p)) < len(names) + len(ROW_NAMES), gate,
                  "wedm_normalize")


# ------------------------------------------------------------------------------------------------ 9. wedm_gae
def test_gae_behind_the_gate(gate):
    """257 environments (two tiles, the second with one live lane) by SCAN_UNROLL + 1 steps (a chunk and a tail), skipping
    after a done and standardising: scan, fold and apply.  The reward block is the gated input, and with it the two done
    flags (``valid`` and the done row follow those alone).  The control is a twin problem reading the same input buffers."""
    flags, N, T = SKIP_AFTER_DONE | NORMALIZE, 257, SCAN_UNROLL + 1
    gated_inputs = ("reward", "terminated", "truncated")
    p, q = (rollout.Problem(N, T, seed=9) for _ in range(2))
    rollout.Problem(N, T, seed=10).call(flags)   # warm-up
    rng = np.random.default_rng(99)
    host_b = {"reward": np.full((T, p.si), np.nan, dtype=np.float32)}
    host_b["reward"][:, :N] = rng.normal(size=(T, N))
    for name in gated_inputs[1:]:
        host_b[name] = np.full((T, p.si), rollout.FILL, dtype=np.uint8)
        host_b[name][:, :N] = rng.random((T, N)) < 0.2
    dev_b = {name: torch.from_numpy(a).to(DEV) for name, a in host_b.items()}
    for name in gated_inputs:
        q.inputs[name] = p.inputs[name]
    p.host.update(host_b)
    want_b, want_a = p.expect(flags), q.expect(flags)
    same = [name for name in p.outputs if not _bytes_differ(want_a[name], want_b[name])]
    assert not same, f"A's and B's definitions agree in {same}"

    def write_b():
        for name in gated_inputs:
            p.inputs[name].t.copy_(dev_b[name])

    def outputs_equal(problem, want):
        return [name for name, b in problem.outputs.items() if not same_bits(b.t, want[name])] == []

    gated(gate, write_b, lambda: p.call(flags), lambda: q.call(flags))
    assert p.differences(want_b) == [], "wedm_gae behind the gate"   # outputs, inputs (B now), every guard band
    assert all(b.bands_intact() for b in q.outputs.values())
    check_control(outputs_equal(q, want_a), any(same_bits(b.t, want_b[name]) for name, b in q.outputs.items()), gate, "wedm_gae")


# ------------------------------------------------------------------------------------------------ 10. wedm_policy_head
def test_policy_head_behind_the_gate(gate):
    """257 rows (a block of 256 and a block with one live lane) of 9 modes: SAMPLE, then EVALUATE of the draw, then BACKWARD,
    as one gated sequence; ``params`` is the gated input.  The control is a twin problem reading the same ``params``."""
    rows, M = 257, 9
    p, q = (head.Problem(rows, M, seed=10) for _ in range(2))
    warm = head.Problem(rows, M, seed=11)
    kw = dict(seed=0x123456789ABCDEF, t=2 ** 32 + 5, env_id_offset=2 ** 32 - 7)
    q.blocks["params"] = p.blocks["params"]
    params_b = random_params(np.random.default_rng(100), rows, M, 0)
    dev_b = torch.from_numpy(params_b).to(DEV)
    p.host["params"] = params_b

    def sequence(problem):
        def go():
            problem.call(SAMPLE, **kw)
            problem.call(EVALUATE)
            problem.call(BACKWARD)
        return go

    def define(problem):
        """The host's blocks after the three calls."""
        problem.adopt(problem.expect(problem.definition(SAMPLE, **kw)))
        problem.adopt(problem.expect(problem.definition(EVALUATE)))
        problem.adopt(problem.expect(problem.definition(BACKWARD, g_entropy=problem.host["g_entropy"])))

    define(p)
    define(q)
    written = head.SAMPLED + ("grad_params",)
    same = [name for name in written if not _bytes_differ(p.host[name], q.host[name])]
    assert not same, f"A's and B's definitions agree in {same}"
    sequence(warm)()   # warm-up
    gated(gate, lambda: p.blocks["params"].t.copy_(dev_b), sequence(p), sequence(q))
    assert p.differences() == [], "wedm_policy_head behind the gate"   # every block (params holds B), every guard band
    assert all(b.bands_intact() for b in q.blocks.values())
    check_control(all(same_bits(q.blocks[name].t, q.host[name]) for name in written),
                  any(same_bits(q.blocks[name].t, p.host[name]) for name in written), gate, "wedm_policy_head")


# ------------------------------------------------------------------------------------------------ 11. two handles at once
GRID = dict(wire_params=WireModuleParameters(segment_len=80.0 / (N_SEG + 0.5)))


def _pair(binding, kernel, lanes, seed):
    gpu, cpu = make(DEV, N_ENVS, binding, **GRID), make("cpu", N_ENVS, binding, **GRID)
    assert gpu.n_segments == N_SEG
    gpu.set_kernel(kernel, lanes)
    return gpu, cpu, scenario(gpu, seed=seed), scenario(cpu, seed=seed)


# the first handle: every binding at once (rows of every kind bound: the library runs kernel 1, and refuses the served kernel,
# which has no form for them), and the served kernel (9, 8) on a plain handle
@pytest.mark.parametrize("binding,kernel,lanes,ran", [("all", 0, 0, "wedm_step_global"), ("plain", 9, 8, "wedm_step_served")],
                         ids=["all", "served8"])
def test_two_handles_on_two_side_streams(gate, binding, kernel, lanes, ran):
    """Two environments of 100 x 99 with different seeds, the second on the two-lane register kernel, each on a side stream
    of its own; launches of 1, 7 and 290 us enqueued in turn with no synchronisation, torch work on the default stream
    meanwhile.  After one synchronise each equals its oracle twin on every byte of every block."""
    first, second = _pair(binding, kernel, lanes, 11), _pair("plain", 7, 2, 12)
    streams = [gate.stream, torch.cuda.Stream(device=DEV)]   # two side streams in all, as in every test here
    try:
        noise = torch.randn(512, 512, device=DEV)
        torch.cuda.synchronize()
        for us in (1, 7, 290):
            for (gpu, _, act, _), S in zip((first, second), streams):
                with torch.cuda.stream(S):
                    gpu.step_many(act, us)
            noise = (noise @ noise) * 1e-3
        torch.cuda.synchronize()
        assert ran in first[0]._backend.last_kernel() and "wedm_step_regs<2>" in second[0]._backend.last_kernel()
        for which, (gpu, cpu, _, act) in (("first", first), ("second", second)):
            for us in (1, 7, 290):
                cpu.step_many(act, us)
            assert_same(everything(gpu), everything(cpu), f"the {which} handle")
            assert int(cpu.state.spark_count.sum()) > 0
        assert _bytes_differ(first[1].state.f64, second[1].state.f64)
    finally:
        first[0].close()
        second[0].close()


def test_a_handle_handed_from_one_stream_to_another_through_an_event(gate):
    """Stepped on S1 behind the gate, an event, `S2.wait_event`, stepped on S2: the twin's result.  (Without the wait the
    race is the caller's, and nothing is asserted about it.)"""
    gpu, cpu, act_g, act_c = _pair("plain", 7, 2, 13)
    S1, S2 = gate.stream, torch.cuda.Stream(device=DEV)
    try:
        torch.cuda.synchronize()
        handed = torch.cuda.Event()
        with torch.cuda.stream(S1):
            gate.close()
            gpu.step_many(act_g, 290)
            handed.record()
        S2.wait_event(handed)
        with torch.cuda.stream(S2):
            gpu.step_many(act_g, 290)
        assert not handed.query(), f"the first launch was over before the second was enqueued: the {gate} did not hold"
        torch.cuda.synchronize()
        for _ in range(2):
            cpu.step_many(act_c, 290)
        assert_same(everything(gpu), everything(cpu), "handed over")
        assert int(cpu.state.spark_count.sum()) > 0
    finally:
        gpu.close()


# ------------------------------------------------------------------------------------------------ 12. the whole stack
STACK_T = 4


def _stack():
    """The scenario of tests/test_policy_head.py's test through the vector adapter and the rollout buffer, with an
    observation and reward normaliser on the adapter: (the adapter, a function that runs STACK_T control steps and `finish`
    and returns everything to compare)."""
    n, T = 64, STACK_T
    vec = WireEDMVectorEnv(make(DEV, n, "autoreset", "s13"), max_episode_steps=3000, normalizer=Normalizer())
    ph = PolicyHead(vec, modes=(5, 9, 13), bounds={"servo": (-0.2, 0.4), "ON_time": (1.0, 4.0), "OFF_time": (20.0, 60.0)}, seed=101)
    buf = RolloutBuffer(vec, T, extras={"log_prob": torch.float32})
    gen = torch.Generator(device=DEV).manual_seed(4)
    params = torch.randn(T, n, ph.param_dim, generator=gen, device=DEV)
    values = torch.randn(T + 1, n, generator=gen, device=DEV)
    first, _ = vec.reset(seed=31)
    first = first.clone()
    vec.env.state.workpiece_position = torch.linspace(10.4, 25.0, n, dtype=torch.float64, device=DEV)
    vec.env.state.wire_position = 10.0

    def run(after_each=lambda: None):
        obs = first
        for t in range(T):
            out = ph.sample(params[t])
            after_each()
            nxt, reward, term, trunc, _ = vec.step(out.action)
            after_each()
            buf.add(obs, ph.stored(out), values[t], reward, term, trunc, log_prob=out.log_prob)
            after_each()
            obs = nxt.clone()   # (the normalised observation is the normaliser's cached output: valid until the next step)
        buf.finish(values[T])
        after_each()

    vec.results = lambda: ({k: v.detach().cpu().clone() for k, v in buf.flat().items()},
                           {"stats": vec.normalizer.stats.cpu().clone(),
                            **{k: v.cpu().clone() for k, v in vec.normalizer.rows.items()}}, everything(vec.env))
    return vec, run


def test_the_whole_stack_runs_ahead_on_a_side_stream(gate):
    """64 environments x 13 segments with in-kernel autoreset, four control steps driven by the policy head, stored in the
    rollout buffer, observation and reward normalised, then `finish`: enqueued on a side stream behind one gate with
    synchronising calls made errors, against the same sequence on the default stream with a synchronise after every call."""
    ref_vec, ref_run = _stack()
    ref_run(torch.cuda.synchronize)
    want = ref_vec.results()
    vec, run = _stack()
    S = gate.stream
    S.wait_stream(torch.cuda.current_stream())
    done = torch.cuda.Event()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.stream(S):
            gate.close()
            run()
            done.record()
        happened = done.query()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert not happened, f"the sequence returned only after the {gate} had ended: something in it waited"
    assert done.query()
    got = vec.results()
    vec.env.check_errors()
    for k in want[0]:
        assert same_bits(got[0][k], want[0][k]), f"flat()[{k!r}]"
    for k in want[1]:
        assert same_bits(got[1][k], want[1][k]), f"normaliser {k}"
    assert_same(got[2], want[2], "the environment's blocks")
    flat = want[0]
    assert bool((flat["terminated"] | flat["truncated"]).any()) and float(flat["reward"].abs().sum()) > 0
    assert float(want[1]["stats"][_abi.NM_COUNT, 0]) > 64 * STACK_T   # the reset's observation and every step's
    ref_vec.close()
    vec.close()
