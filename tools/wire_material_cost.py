#!/usr/bin/env python
"""Cost of a per-environment wire material (wedm_bind_wire_material), rows bound against unbound, in alternating rounds
on environments of the same seed.  The bound rows hold brass -- the configuration's material -- for every environment,
so both sides follow the same trajectories and the difference is the MAT instantiation alone.

  configs4: BASELINE configs[4] as rank 5 of 8 sees it (16 384 environments, per-environment workpiece height / wire
            diameter / current mode, fused launches of 1000 us) -- kernel 2 on both sides;
  headline: BASELINE configs[2] (65 536 environments x 128 segments, uniform geometry) -- the automatic choice on both
            sides: kernel 7 unbound, kernel 2's MAT form bound (the rows need per-environment geometry rows).

    python tools/wire_material_cost.py [--rounds 5] [--launches 10] [--out profiles/r4/wire_material_cost.jsonl]

Prints one JSON line per workload and writes them to --out."""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from env_params_cost import measure  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r4" / "wire_material_cost.jsonl"))
    args = ap.parse_args()

    import bench
    from sparc_amd import EnvironmentConfig, WireEDMEnv, WireModuleParameters

    lines = []
    n_sub = 1000
    # ---- configs[4], rank 5 of 8
    n, rank, world = 16384, 5, 8
    h, d, mode = bench.config5_draws(world * n, rank * n, (rank + 1) * n)
    envs = {}
    for key, rows in (("unbound_k2", False), ("bound_k2", True)):
        kw = dict(workpiece_height=h, wire_diameter=d, env_id_offset=rank * n,
                  config=EnvironmentConfig(target_cutting_distance=5000.0))
        if rows:
            kw["wire_material"] = ["brass"] * n
        env = WireEDMEnv(num_envs=n, device="cuda:0", **kw)
        env.reset(seed=1234)
        env.set_kernel(2)
        envs[key] = (env, env.make_action(0.1, 80.0, mode, 3.0, 80.0))
    med, raw = measure(envs, args.rounds, args.launches, n, n_sub)
    lines.append({
        "workload": "configs4_rank5of8", "shape": f"{n} x per-env geometry x {n_sub} us",
        "unbound_k2_env_steps_per_s": med["unbound_k2"], "bound_k2_env_steps_per_s": med["bound_k2"],
        "ratio_k2": med["bound_k2"] / med["unbound_k2"],
        "kernels": {k: e._backend.last_kernel() for k, (e, _) in envs.items()}, "rates": raw,
    })
    print(json.dumps(lines[-1]), flush=True)
    del envs
    # ---- configs[2], the headline shape
    n = 65536
    envs = {}
    for key, rows in (("unbound_auto", False), ("bound_auto", True)):
        kw = dict(wire_params=WireModuleParameters(segment_len=0.625))
        if rows:
            kw["wire_material"] = ["brass"] * n
        env = WireEDMEnv(num_envs=n, device="cuda:0", **kw)
        env.reset(seed=1234)
        envs[key] = (env, env.make_action(0.1, 80.0, 5, 3.0, 80.0))
    med, raw = measure(envs, args.rounds, args.launches, n, n_sub)
    lines.append({
        "workload": "configs2_headline", "shape": f"{n} x 128 x {n_sub} us",
        "unbound_env_steps_per_s": med["unbound_auto"], "bound_env_steps_per_s": med["bound_auto"],
        "ratio": med["bound_auto"] / med["unbound_auto"],
        "kernels": {k: e._backend.last_kernel() for k, (e, _) in envs.items()}, "rates": raw,
    })
    print(json.dumps(lines[-1]), flush=True)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
