#!/usr/bin/env python
"""Cost of the sensor model as one call (wedm_sensor) against the same formula as a float64 torch composition with
``torch.randn`` and a rolled ring -- what a user could write without the call --, in the same process and build, in
alternating rounds, timed with event pairs, medians.  65 536 environments, 16 source columns in one plane, three sensors:

  identity   16 identity channels (the torch side is one ``index_select``);
  all_L1     16 channels with calibration, noise, quantisation and saturation, no delay (ring of 1);
  all_L8     the same with a delay of up to 7 calls per channel (ring of 8).

The torch composition takes the episode's gain, offset and delay as tensors drawn beforehand (a user draws them at a reset)
and pays for the per-call part: roll the ring, gather the delayed sample, scale, shift, ``randn``, round, clamp, cast.  Its
bits are torch's: there is nothing to compare bit for bit.

  step       `WireEDMVectorEnv.step` at 65 536 x 128 segments (resets inside the kernel, pulse and signal columns) with a
             16-column sensor (every stage on, ring of 4, ``privileged="all"``) and without one, alternating; the adapter
             without a sensor runs the code of the commit before the sensor, so its rounds' spread is that step's own.

    python tools/sensor_cost.py [--rounds 7] [--out profiles/r22/sensor_cost.jsonl]

Prints one JSON line per workload (every sample in it) and writes them to ``--out`` and a table beside it (``.txt``)."""
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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r22" / "sensor_cost.jsonl"))
    args = ap.parse_args()

    import numpy as np
    import torch

    from sparc_amd import Channel, Sensor, WireEDMEnv, WireEDMVectorEnv, WireModuleParameters, _abi, _lib
    from sparc_amd.sensor import MEASURABLE_OBS_NAMES, device_sensor
    from tests._sensor_common import T0, Problem, channel_table

    dev, N, C = "cuda:0", 65536, 16
    SN = _abi.SN
    lines = []
    for name, kind, L in (("identity", "identity", 1), ("all_L1", "all", 1), ("all_L8", "all", 8)):
        rng = np.random.default_rng(1)
        chan, route = channel_table(rng, C, C, L, kind)
        p = Problem(rng, N, (C,), C, L, pad=0, table=(chan, route))
        p.view(p.buf, "first")[:] = 0   # a running episode: the ring is in use
        p.view(p.buf, "pos")[:] = 0
        p.view(p.buf, "age")[:] = L - 1
        buf = torch.from_numpy(p.buf).to(dev)
        desc = p.desc(buf.data_ptr(), T0)
        off, dt, shape = p.layout["plane0"]
        src = buf[off: off + int(np.prod(shape)) * 4].view(torch.float32).view(*shape)
        ring = [torch.zeros((L, C, N), dtype=torch.float32, device=dev)]
        env_index = torch.arange(N, device=dev)
        gain = [1.0 + float(chan[SN.GAIN_SPREAD, c]) * (2.0 * torch.rand(N, dtype=torch.float64, device=dev) - 1.0) for c in range(C)]
        offs = [float(chan[SN.OFFSET_SPREAD, c]) * (2.0 * torch.rand(N, dtype=torch.float64, device=dev) - 1.0) for c in range(C)]
        delay = [torch.randint(0, int(route[1, c]) + 1, (N,), device=dev) for c in range(C)]
        sources = torch.from_numpy(route[0].astype(np.int64)).to(dev)

        def composition():
            if kind == "identity":
                return src.index_select(0, sources)
            if L > 1:
                ring[0] = torch.roll(ring[0], 1, 0)
                ring[0][0] = src
            outs = []
            for c in range(C):
                s = int(route[0, c])
                x = src[s] if L == 1 else ring[0][delay[c], s, env_index]
                y = x.to(torch.float64) * gain[c] + offs[c]
                y = y + float(chan[SN.SIGMA, c]) * torch.randn(N, dtype=torch.float64, device=dev)
                lsb = float(chan[SN.LSB, c])
                y = (lsb * torch.round(y / lsb)).clamp(float(chan[SN.LO, c]), float(chan[SN.HI, c]))
                outs.append(y.to(torch.float32))
            return torch.stack(outs)

        work = {"a": lambda: device_sensor(desc, dev), "b": composition}
        for fn in work.values():
            for _ in range(5):
                fn()
        ms = {k: [] for k in work}
        for _ in range(args.rounds):
            for k, fn in work.items():
                ms[k].append(timed(fn, 50))
        med = {k: statistics.median(v) for k, v in ms.items()}
        ring_bytes = 4 * N * C * 2 if L > 1 else 0   # the slot written (C rows), and at most one delayed sample per channel read
        lines.append({"workload": name, "num_envs": N, "channels": C, "ring_len": L, "a_ms": med["a"], "b_ms": med["b"],
                      "b_over_a": med["b"] / med["a"], "spread_a_ms": max(ms["a"]) - min(ms["a"]), "spread_b_ms": max(ms["b"]) - min(ms["b"]),
                      "source_and_out_bytes": 4 * N * C * 2, "ring_bytes": ring_bytes, "build_id": _lib.build_id(), "ms": ms})
        print(json.dumps(lines[-1]), flush=True)
        del buf, src, ring, gain, offs, delay

    # ---- the adapter's step with and without a sensor
    wire = WireModuleParameters(segment_len=0.625)

    def sensor():
        spec = dict(sigma=0.3, gain_spread=0.05, offset_spread=0.2, lsb=0.125, lo=-1e6, hi=1e6)
        chans = [Channel(n, max_delay=3 if i % 2 else 1, **spec) for i, n in enumerate(MEASURABLE_OBS_NAMES)]
        chans += [Channel(n, name=f"second.{n}", max_delay=2, **spec) for n in MEASURABLE_OBS_NAMES[:7]]
        return Sensor(chans, privileged="all", seed=3)

    vecs = {}
    for name, make in (("plain", lambda: None), ("sensor", sensor)):
        env = WireEDMEnv(num_envs=N, device=dev, wire_params=wire, autoreset=True, reward="progress", pulse_stats=True, signal_stats=True)
        vec = WireEDMVectorEnv(env, max_episode_steps=3000, sensor=make())
        vec.reset(seed=1)
        act = env.make_action(0.1, 80.0, 5, 3.0, 80.0)
        for _ in range(3):
            vec.step(act)
        vecs[name] = (vec, act)
    torch.cuda.synchronize()
    step = {k: [] for k in vecs}
    for _ in range(args.rounds):
        for k, (vec, act) in vecs.items():
            step[k].append(timed(lambda: vec.step(act), 6))
    med = {k: statistics.median(v) for k, v in step.items()}
    lines.append({"workload": "step", "num_envs": N, "segments": 128, "channels": 16, "columns_out": len(vecs["sensor"][0].obs_names),
                  **{f"{k}_ms": v for k, v in med.items()}, "sensor_added_ms": med["sensor"] - med["plain"],
                  "spread_plain_ms": max(step["plain"]) - min(step["plain"]), "build_id": _lib.build_id(), "ms": step})
    print(json.dumps(lines[-1]), flush=True)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("".join(json.dumps(line) + "\n" for line in lines))
    s = lines[-1]
    rows = "".join(
        f"  {c['workload']:9s} wedm_sensor {c['a_ms'] * 1e3:9.2f} us (spread {c['spread_a_ms'] * 1e3:6.2f})   torch float64 "
        f"{c['b_ms'] * 1e3:9.2f} us (spread {c['spread_b_ms'] * 1e3:6.2f})   b / a {c['b_over_a']:7.2f}   ring traffic "
        f"{c['ring_bytes'] / 1e6:.1f} MB, sources and output {c['source_and_out_bytes'] / 1e6:.1f} MB\n" for c in lines[:-1])
    out.with_suffix(".txt").write_text(
        f"wedm_sensor against a float64 torch composition (torch.randn, rolled ring), MI355X, build {s['build_id']}\n"
        f"event pairs, {args.rounds} alternating rounds, medians (spread = max - min of the rounds)\n\n"
        f"the call alone, {N} environments, 16 source columns, 16 channels (50 calls per sample)\n{rows}\n"
        f"WireEDMVectorEnv.step, {N} x 128, pulse and signal columns, in-kernel autoreset (6 steps per sample)\n"
        f"  without a sensor                            {s['plain_ms']:9.4f} ms   spread {s['spread_plain_ms']:.4f} ms\n"
        f"  16 channels, ring of 4, privileged=\"all\"    {s['sensor_ms']:9.4f} ms   ({s['sensor_added_ms'] * 1e3:+.1f} us, "
        f"{s['columns_out']} columns out)\n")


if __name__ == "__main__":
    main()
