"""The two waves of a SIMD in wedm_step_regs<2, *> take turns in issue priority (sparc_amd/csrc/wedm_k_regs.h: the favour
changes sides once, half way through a launch): every microsecond passes scalar branches over `s_setprio`, under a bit the
wave forms by itself and the loop's counter.  Priority cannot change a result; a branch written wrongly can.  Kernel 7
with two lanes per environment runs against the CPU oracle, every state block bit for bit, after each launch of 1, 7, 8, 9,
63, 65 and 400 microseconds in sequence (slices of 8 and of 64 microseconds end inside launches and between them), on

* batches of 32 environments (one wave, no partner), 160 (one full block and one wave) and 333 (the last block partly dead);
* wires of 128 segments and of 100;
* the reset start and the 12 - 15 um mixed start of tests/test_regs_plain_walk.py;
* the forms plain, pulse, float64 stencil, trace and autoreset.

Kernel 7 with one lane and kernel 12 run once each on the batch of 333: they are not touched.

The oracle runs once per (batch, wire, start, form)."""
from __future__ import annotations

import functools

import pytest

from tests.test_regs_plain_walk import FAMILY, FORM_KW, KEYS, TRACE_SIGNALS, WIRES

BATCHES = (32, 160, 333)
LAUNCHES = (1, 7, 8, 9, 63, 65, 400)
FORMS = ("plain", "pulse", "f64", "trace", "autoreset")
CASES = (
    [((7, 2), n, n_seg, start, form) for n in BATCHES for n_seg in (128, 100) for start in ("reset", "mixed") for form in FORMS]
    + [(k, 333, 128, "mixed", "plain") for k in ((7, 1), (12, 0))]
)


def make_env(n, n_seg, form, **kw):
    from sparc_amd import EnvironmentConfig, WireEDMEnv, WireModuleParameters

    env = WireEDMEnv(num_envs=n, wire_params=WireModuleParameters(segment_len=WIRES[n_seg]),
                     config=EnvironmentConfig(target_cutting_distance=5000.0), **FORM_KW[form], **kw)
    assert env.n_segments == n_seg
    return env


def start_state(env, n, start):
    """The starts of tests/test_regs_plain_walk.py for a batch of n."""
    import torch

    env.reset(seed=1111)
    if start == "reset":
        return
    idx = torch.arange(n)
    gap = 12.0 + (idx % 4).double()   # 12 - 15 um
    env.state.wire_position = 10.0
    env.state.workpiece_position = 10.0 + gap
    # a quarter of the batch reaches its target after the first craters: frozen (or re-initialised) environments beside live ones
    env.state.target_position = torch.where(idx % 4 == 0, 10.0 + gap + 0.0005, 5000.0)
    hot = env.state.wire_temperature
    hot[5::17, env.n_segments // 2 - 4:env.n_segments // 2] = 1600.0   # wires that break at the first step


def run(env, n, start, form, after_launch):
    start_state(env, n, start)
    trace = None
    if form == "trace":
        trace = env.bind_trace(TRACE_SIGNALS, every=7, capacity=256, envs=(3, n - 3), wire_temperature=True)
    act = env.make_action(0.1, 80.0, 9, 3.0, 30.0)
    for i, k in enumerate(LAUNCHES):
        env.step_many(act, k)
        after_launch(i)
    if trace is None:
        return None
    return trace.count, {sig: v.cpu() for sig, v in trace.read().items()}


@functools.lru_cache(maxsize=None)
def oracle_run(n, n_seg, start, form):
    from tests._oracle_backend import OracleBackend

    env = make_env(n, n_seg, form, device="cpu", backend=OracleBackend)
    blocks = []
    trace = run(env, n, start, form, lambda i: blocks.append(env.state.clone_blocks()))
    return blocks, trace, int(env.state.spark_count.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,n,n_seg,start,form", CASES,
                         ids=lambda v: "k%d_l%d" % v if isinstance(v, tuple) else str(v))
def test_pair_fair_matches_oracle_after_every_launch(kernel, n, n_seg, start, form):
    import torch

    from tests._compare import assert_blocks_equal

    # (pulse statistics change no state row: the oracle of the plain form)
    want, want_trace, sparks = oracle_run(n, n_seg, start, "plain" if form == "pulse" else form)
    gpu = make_env(n, n_seg, form, device="cuda:0", pulse_stats=(form == "pulse"))
    gpu.set_kernel(*kernel)

    def check(i):
        torch.cuda.synchronize()
        g = gpu.state.clone_blocks()
        if form == "pulse":
            assert_blocks_equal({k: g[k] for k in KEYS}, {k: want[i][k] for k in KEYS}, n)
            assert torch.equal(g["obs"][:8, :n].cpu(), want[i]["obs"][:, :n].cpu()), i
        else:
            assert_blocks_equal(g, want[i], n)
        name = gpu._backend.last_kernel()
        assert name.startswith(FAMILY[kernel]), (i, name)
        assert ("[f64 stencil]" in name) == (form == "f64") and ("[pulse]" in name) == (form == "pulse"), (i, name)

    got_trace = run(gpu, n, start, form, check)
    if form == "trace":
        assert got_trace[0] == want_trace[0] > 0
        for sig, w in want_trace[1].items():
            g = got_trace[1][sig]
            same = (g == w) | ((g != g) & (w != w))
            assert bool(same.all()), (sig, int((~same).sum()))
    # the narrow gaps did what they are for: sparks, so general microseconds between quiet ones
    if start == "mixed":
        assert sparks > n // 2
