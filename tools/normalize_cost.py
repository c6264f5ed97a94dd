#!/usr/bin/env python
"""Cost of running normalisation (wedm_normalize) in `WireEDMVectorEnv.step`, with a `Normalizer` against without, in
alternating rounds on environments of the same seed at the headline batch (65 536 environments x 128 segments, control
steps of 1000 us, autoreset and the progress reward in the kernel).  Both sides follow the same trajectories: the
normaliser reads the physics and writes none of it.

  obs8:       the environment's 8 observation columns (C = 9);
  obs16_bins8: pulse and signal statistics (16 columns) plus an 8-bin wire profile (20 rows): C = 37.  Both sides pay for the
               profile launch; the difference is the normaliser alone.

Also times the normaliser's call by itself on the last step's blocks (its three launches back to back, no step between).

    python tools/normalize_cost.py [--rounds 5] [--steps 10]

Prints one JSON line per workload."""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def timed(fn, count):
    import torch

    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(count):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / count  # ms per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--envs", type=int, default=65536)
    args = ap.parse_args()

    import torch

    from sparc_amd import EnvironmentConfig, Normalizer, WireEDMEnv, WireEDMVectorEnv, WireModuleParameters, _abi, _lib

    n = args.envs
    for name, opts, bins in (("obs8", {}, None), ("obs16_bins8", dict(pulse_stats=True, signal_stats=True), 8)):
        vecs = {}
        for key in ("plain", "normalized"):
            env = WireEDMEnv(num_envs=n, device="cuda:0", autoreset=True, reward="progress",
                             wire_params=WireModuleParameters(segment_len=0.625),
                             config=EnvironmentConfig(target_cutting_distance=5000.0), **opts)
            kw = {} if bins is None else dict(wire_profile_bins=bins)
            if key == "normalized":
                kw["normalizer"] = Normalizer()
            vec = WireEDMVectorEnv(env, max_episode_steps=50000, **kw)
            vec.reset(seed=1234)
            act = env.make_action(0.1, 80.0, 5, 3.0, 80.0)
            for _ in range(3):  # warm-up: code objects loaded, plans made, caches allocated
                vec.step(act)
            vecs[key] = (vec, act)
        torch.cuda.synchronize()
        ms = {k: [] for k in vecs}
        for _ in range(args.rounds):
            for k, (vec, act) in vecs.items():
                ms[k].append(timed(lambda: vec.step(act), args.steps))
        med = {k: statistics.median(v) for k, v in ms.items()}
        vec, act = vecs["normalized"]
        _, reward, term, trunc, _ = vec.step(act)
        planes = vec._planes()
        norm = vec.normalizer
        call = [timed(lambda: norm.normalize(planes, reward=reward, terminated=term, truncated=trunc), 50)
                for _ in range(args.rounds)]
        # the two phases by themselves: the descriptor of the last call, with one phase named (REDUCE: one launch, the
        # tree; APPLY: two, the fold and the outputs)
        desc, phases = norm._desc, {}
        for phase, bit in (("reduce", _abi.NORM_REDUCE), ("apply", _abi.NORM_APPLY)):
            desc.flags = _abi.NORM_UPDATE | _abi.NORM_STEP | bit
            phases[phase] = statistics.median(timed(lambda: vec.env._backend.normalize(desc), 50) for _ in range(args.rounds))
        print(json.dumps({
            "workload": name, "shape": f"{n} x 128 x 1000 us", "columns": len(vec.normalizer.columns),
            "plain_ms_per_step": med["plain"], "normalized_ms_per_step": med["normalized"],
            "added_ms": med["normalized"] - med["plain"], "added_fraction": med["normalized"] / med["plain"] - 1.0,
            "call_alone_ms": statistics.median(call), "reduce_alone_ms": phases["reduce"], "apply_alone_ms": phases["apply"], "kernel": vec.env._backend.last_kernel(), "build_id": _lib.build_id(),
            "ms": ms, "call_ms": call,
        }))
        del vecs, vec


if __name__ == "__main__":
    main()
