#!/usr/bin/env python
"""Cost of the shaped reward as one call (wedm_reward) against the same formula as a float64 torch expression -- what a user
writes as ``WireEDMVectorEnv(env, reward=callable)`` --, in the same process and build, in alternating rounds, timed with
event pairs, medians.  65 536 environments, all ten terms on:

  a  the call, with ``terms_out``, a mask and a restart mask;
  b  the torch composition on the same blocks (no mask: the callable path has none; its progress term takes the ``prev``
     tensor the adapter hands it);
  c  `WireEDMVectorEnv.step` at 65 536 x 128 segments (resets inside the kernel, pulse and signal statistics) with the
     `ShapedReward`, with the torch callable, and with the kernel's own progress reward, alternating.

Before timing, a and b run once on the same rows and ``same_bits`` records whether their float32 rewards are equal bit for
bit (in c: the rewards of one step of the two adapters).

    python tools/reward_cost.py [--rounds 7] [--out profiles/r21/reward_cost.jsonl]

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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r21" / "reward_cost.jsonl"))
    args = ap.parse_args()

    import numpy as np
    import torch

    from sparc_amd import ShapedReward, WireEDMEnv, WireEDMVectorEnv, WireModuleParameters, _abi, _lib
    from sparc_amd.reward import device_reward
    from tests._reward_common import ALL_ON, GAP_FLOOR, TMAX_CEILING, Problem

    dev, N = "cuda:0", 65536
    F64, I8, PULSE, SIG = _abi.F64, _abi.I8, _abi.PULSE, _abi.SIG
    W = ALL_ON

    def composition(f64, i8, pulse, sig, before, floor, ceiling):
        """The ten terms in term order as a float64 torch expression over the state rows; float32 out."""
        n = before.shape[0]
        r = W[0] * (f64[F64.WORKPIECE_POS, :n] - before)
        r = r + W[1]
        r = r + W[2] * (i8[I8.WIRE_BROKEN, :n] != 0).to(torch.float64)
        r = r + W[3] * (i8[I8.TARGET_REACHED, :n] != 0).to(torch.float64)
        r = r + W[4] * pulse[PULSE.SPARK_ACC, :n].to(torch.float64)
        r = r + W[5] * pulse[PULSE.SHORT_ACC, :n].to(torch.float64)
        r = r + W[6] * pulse[PULSE.SHORT_STEPS_ACC, :n].to(torch.float64)
        r = r + W[7] * sig[SIG.ENERGY_ACC, :n]
        has = sig[SIG.SAMPLES_ACC, :n] > 0
        gmin, peak = sig[SIG.GAP_MIN_ACC, :n], sig[SIG.TMAX_PEAK_ACC, :n]
        r = r + W[8] * torch.where(has & (floor > gmin), floor - gmin, 0.0)
        r = r + W[9] * torch.where(has & (peak > ceiling), peak - ceiling, 0.0)
        return r.to(torch.float32)

    # ---- a and b on one arena
    rng = np.random.default_rng(1)
    p = Problem(rng, N, masked=True, restart=True)
    buf = torch.from_numpy(p.buf).to(dev)

    def view(name):
        off, dt, shape = p.layout[name]
        t = buf[off: off + int(np.prod(shape)) * dt.itemsize].view(getattr(torch, np.dtype(dt).name))
        return t.view(*shape)

    desc = p.desc(buf.data_ptr())
    plain = p.desc(buf.data_ptr())
    plain.mask = plain.restart = None
    blocks = (view("f64"), view("i8"), view("pulse"), view("sig"), view("pos_before"))
    call = lambda: device_reward(desc, dev)                                  # noqa: E731
    torch_call = lambda: composition(*blocks, GAP_FLOOR, TMAX_CEILING)       # noqa: E731
    device_reward(plain, dev)
    got, want = view("reward_out").clone(), torch_call()
    torch.cuda.synchronize()
    same_call = bool(torch.equal(got.view(torch.int32), want.view(torch.int32)))
    work = {"a": call, "b": torch_call}
    for fn in work.values():
        for _ in range(5):
            fn()
    ms = {k: [] for k in work}
    for _ in range(args.rounds):
        for k, fn in work.items():
            ms[k].append(timed(fn, 100))
    med = {k: statistics.median(v) for k, v in ms.items()}
    lines = [{"workload": "call", "num_envs": N, "terms": 10, "a_ms": med["a"], "b_ms": med["b"], "b_over_a": med["b"] / med["a"], "same_bits": same_call,
              "spread_a_ms": max(ms["a"]) - min(ms["a"]), "spread_b_ms": max(ms["b"]) - min(ms["b"]),
              "build_id": _lib.build_id(), "ms": ms}]
    print(json.dumps(lines[-1]), flush=True)
    del buf, blocks

    # ---- c: the adapter's step with each reward
    wire = WireModuleParameters(segment_len=0.625)
    floor, ceiling = 12.0, 320.0

    def torch_reward(env, prev):
        st = env.state
        return composition(st.f64, st.i8, st.pulse, st.signal, prev["workpiece_position"], floor, ceiling)

    rewards = {"shaped": lambda: ShapedReward(W[0], W[1], W[2], W[3], W[4], W[5], W[6], W[7], (W[8], floor), (W[9], ceiling)),
               "torch": lambda: torch_reward, "kernel": lambda: None}
    vecs = {}
    for name, make in rewards.items():
        env = WireEDMEnv(num_envs=N, device=dev, wire_params=wire, autoreset=True, reward="progress", pulse_stats=True,
                         signal_stats=True)
        vec = WireEDMVectorEnv(env, max_episode_steps=3000, reward=make())
        vec.reset(seed=1)
        act = env.make_action(0.1, 80.0, 5, 3.0, 80.0)
        for _ in range(3):
            vec.step(act)
        vecs[name] = (vec, act)
    # the two rewards of the same step are the same numbers
    a, b = vecs["shaped"][0].step(vecs["shaped"][1])[1], vecs["torch"][0].step(vecs["torch"][1])[1]
    vecs["kernel"][0].step(vecs["kernel"][1])
    torch.cuda.synchronize()
    same_step = bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))
    step = {k: [] for k in vecs}
    for _ in range(args.rounds):
        for k, (vec, act) in vecs.items():
            step[k].append(timed(lambda: vec.step(act), 6))
    med = {k: statistics.median(v) for k, v in step.items()}
    lines.append({"workload": "step", "num_envs": N, "segments": 128, **{f"{k}_ms": v for k, v in med.items()},
                  "shaped_added_ms": med["shaped"] - med["kernel"], "torch_added_ms": med["torch"] - med["kernel"],
                  "spread_kernel_ms": max(step["kernel"]) - min(step["kernel"]), "same_bits": same_step, "build_id": _lib.build_id(), "ms": step})
    print(json.dumps(lines[-1]), flush=True)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("".join(json.dumps(line) + "\n" for line in lines))
    c, s = lines
    out.with_suffix(".txt").write_text(
        f"wedm_reward against the float64 torch composition, MI355X, build {c['build_id']}\n"
        f"event pairs, {args.rounds} alternating rounds, medians (spread = max - min of the rounds)\n\n"
        f"the call alone, {N} environments, ten terms on (100 calls per sample)\n"
        f"  a  wedm_reward (terms_out, mask, restart)   {c['a_ms'] * 1e3:9.2f} us   spread {c['spread_a_ms'] * 1e3:.2f} us\n"
        f"  b  torch composition, float64               {c['b_ms'] * 1e3:9.2f} us   spread {c['spread_b_ms'] * 1e3:.2f} us\n"
        f"  b / a                                       {c['b_over_a']:9.2f}   (same float32 bits: {c['same_bits']})\n\n"
        f"WireEDMVectorEnv.step, {N} x 128, pulse and signal statistics, in-kernel autoreset (6 steps per sample)\n"
        f"  kernel's progress reward                    {s['kernel_ms']:9.4f} ms   spread {s['spread_kernel_ms']:.4f} ms\n"
        f"  ShapedReward                                {s['shaped_ms']:9.4f} ms   (+{s['shaped_added_ms'] * 1e3:.1f} us)\n"
        f"  torch callable                              {s['torch_ms']:9.4f} ms   (+{s['torch_added_ms'] * 1e3:.1f} us)\n"
        f"  the two rewards of one step have the same float32 bits: {s['same_bits']}\n")


if __name__ == "__main__":
    main()
