#!/usr/bin/env python
"""Cost of per-interval signal statistics (wedm_bind_signal_stats), block bound against not bound, in alternating rounds
on environments of the same seed.  The block changes no trajectory, so both sides step the same states and the difference
is the SIG instantiation (and, where the plan changes, the kernel).

  configs4: BASELINE configs[4] as rank 5 of 8 sees it (16 384 environments, per-environment workpiece height / wire
            diameter / current mode, fused launches of 1000 us) -- kernel 2 on both sides, and the automatic choice
            without the block for reference;
  headline: BASELINE configs[2] (65 536 environments x 128 segments) -- the automatic choice on both sides: kernel 7
            unbound, kernel 2's SIG form bound.

    python tools/signal_stats_cost.py [--rounds 5] [--launches 10] [--unbound-only]

--unbound-only: the unbound sides alone (what a checkout without the block can also run: its rates in the same session say
whether the unbound launches moved).  Prints one JSON line per workload."""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def measure(envs, rounds, launches, n, n_sub):
    import torch

    for env, act in envs.values():  # warm-up: code objects loaded, plans made, the batch past its first control step
        for _ in range(3):
            env.step_many(act, n_sub)
    torch.cuda.synchronize()
    rates = {k: [] for k in envs}
    for _ in range(rounds):
        for k, (env, act) in envs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(launches):
                env.step_many(act, n_sub)
            t1.record()
            t1.synchronize()
            rates[k].append(n * n_sub * launches / (t0.elapsed_time(t1) * 1e-3))
    return {k: statistics.median(v) for k, v in rates.items()}, rates


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--unbound-only", action="store_true")
    args = ap.parse_args()

    import bench
    from sparc_amd import EnvironmentConfig, WireEDMEnv, WireModuleParameters, _lib

    build = _lib.build_id()
    sig = not args.unbound_only
    n_sub = 1000
    # ---- configs[4], rank 5 of 8
    n, rank, world = 16384, 5, 8
    h, d, mode = bench.config5_draws(world * n, rank * n, (rank + 1) * n)
    envs = {}
    for key, bound, kernel in (("unbound_k2", False, 2), ("bound_k2", True, 2), ("unbound_auto", False, 0)):
        if bound and not sig:
            continue
        env = WireEDMEnv(num_envs=n, device="cuda:0", workpiece_height=h, wire_diameter=d, env_id_offset=rank * n,
                         config=EnvironmentConfig(target_cutting_distance=5000.0), **({"signal_stats": True} if bound else {}))
        env.reset(seed=1234)
        env.set_kernel(kernel)
        envs[key] = (env, env.make_action(0.1, 80.0, mode, 3.0, 80.0))
    med, raw = measure(envs, args.rounds, args.launches, n, n_sub)
    out = {"workload": "configs4_rank5of8", "shape": f"{n} x per-env geometry x {n_sub} us", "build_id": build,
           "unbound_k2_env_steps_per_s": med["unbound_k2"], "unbound_auto_env_steps_per_s": med["unbound_auto"]}
    if sig:
        out.update(bound_k2_env_steps_per_s=med["bound_k2"], ratio_k2=med["bound_k2"] / med["unbound_k2"],
                   ratio_to_auto=med["bound_k2"] / med["unbound_auto"])
    out.update(kernels={k: e._backend.last_kernel() for k, (e, _) in envs.items()}, rates=raw)
    print(json.dumps(out), flush=True)
    del envs
    # ---- configs[2], the headline
    n = 65536
    envs = {}
    for key, bound in (("unbound_auto", False), ("bound_auto", True)):
        if bound and not sig:
            continue
        env = WireEDMEnv(num_envs=n, device="cuda:0", wire_params=WireModuleParameters(segment_len=0.625),
                         **({"signal_stats": True} if bound else {}))
        env.reset(seed=1234)
        envs[key] = (env, env.make_action(0.1, 80.0, 5, 3.0, 80.0))
    med, raw = measure(envs, args.rounds, args.launches, n, n_sub)
    out = {"workload": "configs2_headline", "shape": f"{n} x 128 x {n_sub} us", "build_id": build,
           "unbound_env_steps_per_s": med["unbound_auto"]}
    if sig:
        out.update(bound_env_steps_per_s=med["bound_auto"], ratio=med["bound_auto"] / med["unbound_auto"])
    out.update(kernels={k: e._backend.last_kernel() for k, (e, _) in envs.items()}, rates=raw)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
