#!/usr/bin/env python
"""Cost of the pulse statistics (wedm_bind_pulse_stats) on the headline launch: BASELINE configs[2] (65 536 environments x
128 segments, fused launches of 1000 us, fresh reset, the quickstart action) on kernel 7, with the block bound (the PULSE
instantiation) and unbound, in alternating rounds on two environments of the same seed.

    python tools/pulse_cost.py [--rounds 5] [--launches 20]

Prints one JSON line: env-steps/s of both, their ratio, the kernels' names and the published spark counts."""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--num-envs", type=int, default=65536)
    args = ap.parse_args()

    import torch

    from sparc_amd import WireEDMEnv, WireModuleParameters

    n, n_sub = args.num_envs, 1000
    envs = {}
    for pulse in (False, True):
        env = WireEDMEnv(num_envs=n, device="cuda:0", wire_params=WireModuleParameters(segment_len=0.625), pulse_stats=pulse)
        env.reset(seed=1234)
        env.set_kernel(7)
        envs[pulse] = (env, env.make_action(0.1, 80.0, 5, 3.0, 80.0))
    for env, act in envs.values():  # warm-up: code objects loaded, plans made, the batch past its first control step
        for _ in range(3):
            env.step_many(act, n_sub)
    torch.cuda.synchronize()
    rates = {False: [], True: []}
    for _ in range(args.rounds):
        for pulse, (env, act) in envs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.launches):
                env.step_many(act, n_sub)
            t1.record()
            t1.synchronize()
            rates[pulse].append(n * n_sub * args.launches / (t0.elapsed_time(t1) * 1e-3))
    off, on = statistics.median(rates[False]), statistics.median(rates[True])
    env_on = envs[True][0]
    print(json.dumps({
        "shape": f"{n} x 128 x {n_sub} us", "unbound_env_steps_per_s": off, "bound_env_steps_per_s": on, "ratio": on / off,
        "kernel_unbound": envs[False][0]._backend.last_kernel(), "kernel_bound": env_on._backend.last_kernel(),
        "rounds": args.rounds, "launches_per_round": args.launches,
        "rates_unbound": rates[False], "rates_bound": rates[True],
        "mean_spark_pulses_per_interval": float(env_on.get_pulse_statistics()["spark_pulses"].double().mean()),
        "mean_short_pulses_per_interval": float(env_on.get_pulse_statistics()["short_pulses"].double().mean()),
    }))


if __name__ == "__main__":
    main()
