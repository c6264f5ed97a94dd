#!/usr/bin/env python
"""Cost of per-episode domain randomisation in `WireEDMVectorEnv.step`: the adapter's step with
  (a) plain:    no sampler;
  (b) torch:    the three existing samplers (`uniform_param_sampler`, `uniform_material_sampler`, `uniform_geometry_sampler`);
  (c) episode:  `EpisodeSampler` drawing the same names from the same ranges with one launch of `wedm_draw_episode`,
on two workloads: BASELINE configs[4] as rank 5 of 8 sees it (16 384 environments, per-environment workpiece height / wire
diameter / current mode) and 65 536 environments x 128 segments on kernel 2.  In-kernel autoreset, progress reward, fused
launches of 1000 us; no episode ends while the clock runs, so (b) and (c) work under an empty reset mask -- which is what a
step pays most of the time: torch's samplers enqueue the same launches whatever the mask holds, the kernel's lanes return
after reading it.  `draw_all` therefore also times one application to EVERY environment, (b) `_apply_sampler(all)` against
(c) `EpisodeSampler.draw(mask=None)`, outside the step.

Alternating rounds, device events, medians and every sample.  One JSON line per figure, printed and written to --out.

    python tools/episode_sampler_cost.py [--rounds 5] [--steps 10] [--calls 20] [--out profiles/r4/episode_sampler_cost.jsonl]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

PARAMS = {"omega_n": (200.0, 270.0), "zeta": (0.3, 0.45), "plasma_efficiency": (0.08, 0.12),
          "base_convection_coefficient": (12000.0, 16000.0), "debris_removal_efficiency": (0.008, 0.012)}
DIAMETERS = (0.10, 0.15, 0.20, 0.25, 0.30)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r4" / "episode_sampler_cost.jsonl"))
    args = ap.parse_args()

    import dataclasses

    import torch

    import bench
    from sparc_amd import (DielectricModuleParameters, EnvironmentConfig, EpisodeSampler, MechanicsModuleParameters, WireEDMEnv,
                           WireEDMVectorEnv, WireModuleParameters, get_material_db, uniform_geometry_sampler,
                           uniform_material_sampler, uniform_param_sampler)

    dev = "cuda:0"
    brass = get_material_db().get_wire_material("brass")
    # a second material for the table: brass with another conductivity and resistivity (what is drawn is the index)
    other = dataclasses.replace(brass, name="brass-b", thermal_conductivity=brass.thermal_conductivity * 1.1,
                                electrical_resistivity=brass.electrical_resistivity * 0.9)

    # the environments start from the dataclass values of the randomised names
    defaults = {name: float(getattr(owner, name)) for owner in (DielectricModuleParameters(), MechanicsModuleParameters(),
                                                                WireModuleParameters()) for name in PARAMS if hasattr(owner, name)}
    assert set(defaults) == set(PARAMS)

    def events(fn, calls):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(calls):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / calls * 1e3

    def workload(tag):
        if tag == "configs4_rank5of8":
            n, rank, world = 16384, 5, 8
            h, d, mode = bench.config5_draws(world * n, rank * n, (rank + 1) * n)
            return dict(num_envs=n, workpiece_height=h, wire_diameter=d, env_id_offset=rank * n,
                        dynamic_geometry={"max_workpiece_height": 30.0, "wire_diameters": DIAMETERS}), mode, (10.0, 30.0), None
        n = 65536  # 128 segments: the 20 mm workpiece of the default configuration on a 0.625 mm grid
        return dict(num_envs=n, wire_params=WireModuleParameters(segment_len=0.625), wire_diameter=0.25,
                    dynamic_geometry={"max_workpiece_height": 20.0, "wire_diameters": DIAMETERS}), 5, (10.0, 20.0), 2

    lines = []
    for tag in ("configs4_rank5of8", "65536x128_kernel2"):
        kw, mode, heights, kernel = workload(tag)
        n = kw["num_envs"]
        vecs = {}
        for key in ("plain", "torch", "episode"):
            env = WireEDMEnv(device=dev, autoreset=True, reward="progress", wire_material=[brass, other] * (n // 2),
                             env_params={name: defaults[name] for name in PARAMS},
                             config=EnvironmentConfig(target_cutting_distance=5000.0), **kw)
            if kernel is not None:
                env.set_kernel(kernel)
            samplers = {}
            if key == "torch":
                gen = torch.Generator(device=dev).manual_seed(11)
                samplers = dict(param_sampler=uniform_param_sampler(PARAMS, generator=gen),
                                material_sampler=uniform_material_sampler(generator=gen),
                                geometry_sampler=uniform_geometry_sampler(height=heights, generator=gen))
            elif key == "episode":
                samplers = dict(episode_sampler=EpisodeSampler(11, params=PARAMS, materials=True, height=heights, diameters=True))
            vec = WireEDMVectorEnv(env, **samplers)
            env.reset(seed=1234)  # (not vec.reset: every side keeps the constructor's physics and follows the same trajectories)
            vecs[key] = (vec, env.make_action(0.1, 80.0, mode, 3.0, 80.0))
        for vec, act in vecs.values():
            for _ in range(3):
                vec.step(act)
        us = {k: [] for k in vecs}
        for _ in range(args.rounds):
            for k, (vec, act) in vecs.items():
                us[k].append(events(lambda: vec.step(act), args.steps))
        med = {k: statistics.median(x) for k, x in us.items()}
        spread = {k: max(x) - min(x) for k, x in us.items()}
        for vec, _ in vecs.values():
            vec.env.check_errors()
        lines.append({"figure": "vector_step", "workload": tag, "num_envs": n, "n_seg_max": vecs["plain"][0].env.n_segments,
                      "step_plain_us": med["plain"], "step_torch_samplers_us": med["torch"], "step_episode_sampler_us": med["episode"],
                      "added_torch_us": med["torch"] - med["plain"], "added_episode_us": med["episode"] - med["plain"],
                      "spread_between_rounds_us": spread,
                      "kernels": {k: v.env._backend.last_kernel() for k, (v, _) in vecs.items()},
                      "build_id": vecs["plain"][0].env._backend.build_id(), "us": us})
        # one application to every environment, outside the step (the state is not stepped on afterwards)
        everyone = torch.ones(n, dtype=torch.bool, device=dev)
        v_torch, v_episode = vecs["torch"][0], vecs["episode"][0]
        ways = {"torch": lambda: v_torch._apply_sampler(everyone),
                "episode": lambda: v_episode._episode_sampler.draw(v_episode.env, mask=None, reset=False)}
        for fn in ways.values():
            fn()
        us = {k: [] for k in ways}
        for _ in range(args.rounds):
            for k, fn in ways.items():
                us[k].append(events(fn, args.calls))
        med = {k: statistics.median(x) for k, x in us.items()}
        for vec in (v_torch, v_episode):
            vec.env.check_errors()
        lines.append({"figure": "draw_all", "workload": tag, "num_envs": n, "torch_samplers_us": med["torch"],
                      "episode_sampler_us": med["episode"], "torch_over_episode": med["torch"] / med["episode"],
                      "build_id": v_torch.env._backend.build_id(), "us": us})
        del vecs, ways, v_torch, v_episode
        torch.cuda.empty_cache()
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    with out.open("w") as f:
        for line in lines:
            text = json.dumps(line)
            print(text)
            f.write(text + "\n")


if __name__ == "__main__":
    main()
