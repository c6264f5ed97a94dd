"""The register walk (sparc_amd/csrc/wedm_regs_walk.inc) enters a microsecond in one of two ways: PLAIN, for a wave in which
no lane carries current or a plasma heat (the tile masks are constants of the launch), and busy (the masks come from the
lanes' coefficients).  Here the kernels that include that text -- kernel 7 with one and with two lanes per environment, and
the walkers of kernel 12 -- run against the CPU oracle, every state block bit for bit, after each launch of 1, 7, 400 and
1300 microseconds in sequence, on

* wires of 128 segments, of 100 (not a multiple of 8: the wire's last cell lies inside a tile, and some tiles are not
  regular) and of 64 (the chunks of an environment's second lane are empty);
* the reset state's 50 um gap (PLAIN microseconds only, until the first ignitions) and a 12 - 15 um gap (waves alternate
  between the two entries inside one launch), there with frozen environments beside live ones and wires that break at once;
* the forms plain, trace, pulse, float64 stencil and autoreset.

The oracle runs once per (wire, start, form) and is shared by the kernels."""
from __future__ import annotations

import functools

import pytest

N = 333   # not a multiple of a block's environments: the last block is partly dead
LAUNCHES = (1, 7, 400, 1300)
WIRES = {128: 0.625, 100: 0.8, 64: 1.25}   # segments: segment_len
KEYS = ("f64", "i32", "i8", "T", "stats", "reward")   # (the oracle carries no pulse rows: every other block)
TRACE = dict(every=7, capacity=256, envs=(3, N - 3), wire_temperature=True)
TRACE_SIGNALS = ["voltage", "time", "spark_state"]
FORM_KW = {"plain": {}, "trace": {}, "pulse": {}, "f64": dict(stencil_dtype="float64"), "autoreset": dict(autoreset=True)}
FAMILY = {(7, 1): "wedm_step_regs<1>", (7, 2): "wedm_step_regs<2>", (12, 0): "wedm_step_regs_served<"}

REGS = [(7, 1), (7, 2)]
ALL = REGS + [(12, 0)]   # (kernel 12 has the float32 stencil without a trace sample or pulse statistics)
CASES = (
    [(k, n, start, "plain") for k in ALL for n in WIRES for start in ("reset", "mixed")]
    + [(k, n, "mixed", form) for form in ("trace", "pulse", "f64") for k in REGS for n in (128, 100)]
    + [((7, 2), 128, "reset", form) for form in ("trace", "pulse", "f64")]
    + [(k, n, "mixed", "autoreset") for k in ALL for n in (128, 100)]
)


def make_env(n_seg, form, **kw):
    from sparc_amd import EnvironmentConfig, WireEDMEnv, WireModuleParameters

    env = WireEDMEnv(num_envs=N, wire_params=WireModuleParameters(segment_len=WIRES[n_seg]),
                     config=EnvironmentConfig(target_cutting_distance=5000.0), **FORM_KW[form], **kw)
    assert env.n_segments == n_seg
    return env


def start_state(env, start):
    import torch

    env.reset(seed=1111)
    if start == "reset":
        return
    idx = torch.arange(N)
    gap = 12.0 + (idx % 4).double()   # 12 - 15 um
    env.state.wire_position = 10.0
    env.state.workpiece_position = 10.0 + gap
    # a quarter of the batch reaches its target after the first craters: frozen (or re-initialised) environments beside live
    # ones in every wave, the last environment of the odd batch among them
    env.state.target_position = torch.where(idx % 4 == 0, 10.0 + gap + 0.0005, 5000.0)
    hot = env.state.wire_temperature
    hot[5::17, env.n_segments // 2 - 4:env.n_segments // 2] = 1600.0   # wires that break at the first step


def run(env, start, form, after_launch):
    """Step `env` through LAUNCHES from `start`; after_launch(i) after each.  Returns the trace's samples, if the form has one."""
    start_state(env, start)
    trace = env.bind_trace(TRACE_SIGNALS, **TRACE) if form == "trace" else None
    act = env.make_action(0.1, 80.0, 9, 3.0, 30.0)
    for i, k in enumerate(LAUNCHES):
        env.step_many(act, k)
        after_launch(i)
    if trace is None:
        return None
    return trace.count, {sig: v.cpu() for sig, v in trace.read().items()}


@functools.lru_cache(maxsize=None)
def oracle_run(n_seg, start, form):
    """The CPU oracle's blocks after each launch (and the trace), once for every kernel of the case."""
    from tests._oracle_backend import OracleBackend

    env = make_env(n_seg, form, device="cpu", backend=OracleBackend)
    blocks = []
    trace = run(env, start, form, lambda i: blocks.append(env.state.clone_blocks()))
    return blocks, trace, int(env.state.spark_count.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,n_seg,start,form", CASES, ids=lambda v: "k%d_l%d" % v if isinstance(v, tuple) else str(v))
def test_register_walk_matches_oracle_after_every_launch(kernel, n_seg, start, form):
    import torch

    from tests._compare import assert_blocks_equal

    # (pulse statistics change no state row: the oracle of the plain form)
    want, want_trace, sparks = oracle_run(n_seg, start, "plain" if form == "pulse" else form)
    gpu = make_env(n_seg, form, device="cuda:0", pulse_stats=(form == "pulse"))
    gpu.set_kernel(*kernel)

    def check(i):
        torch.cuda.synchronize()
        g = gpu.state.clone_blocks()
        if form == "pulse":
            assert_blocks_equal({k: g[k] for k in KEYS}, {k: want[i][k] for k in KEYS}, N)
            assert torch.equal(g["obs"][:8, :N].cpu(), want[i]["obs"][:, :N].cpu()), i
        else:
            assert_blocks_equal(g, want[i], N)
        name = gpu._backend.last_kernel()
        assert name.startswith(FAMILY[kernel]), (i, name)
        assert ("[f64 stencil]" in name) == (form == "f64") and ("[pulse]" in name) == (form == "pulse"), (i, name)

    got_trace = run(gpu, start, form, check)
    if form == "trace":
        assert got_trace[0] == want_trace[0] > 0
        for sig, w in want_trace[1].items():
            g = got_trace[1][sig]
            same = (g == w) | ((g != g) & (w != w))
            assert bool(same.all()), (sig, int((~same).sum()))
    # the narrow gaps did what they are for: sparks, so busy waves between PLAIN microseconds
    if start == "mixed":
        assert sparks > N // 2
