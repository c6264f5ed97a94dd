#!/usr/bin/env python
"""Cost of `RolloutBuffer.finish` (wedm_gae: advantages, returns, valid mask and standardised advantages of a rollout) against
the same recurrence written as a reversed loop of torch operations in float64 on the same blocks -- what a user writes
without the call, and the only thing to compare against -- in alternating rounds, timed with event pairs, at two shapes:

  wide:  T = 128 steps x N = 65 536 environments (the headline batch);
  long:  T = 2048 steps x N = 4096 environments (the time loop runs in the lane: 16 blocks).

Also times the call's two phases by themselves (SCAN: one launch; APPLY: the fold and the element-wise pass).  The bytes per
second are the algorithmic bytes -- 10 read and 9 written per element by the scan, 8 more with normalisation -- over the
median time.

    python tools/gae_cost.py [--rounds 5]

Prints one JSON line per shape."""
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


def torch_loop(buf, last_value):
    """The recurrence of `wedm_gae` as torch operations, float64, one reversed Python loop: about ten launches per step."""
    import torch

    s, T = buf.stored, buf.num_steps
    r, v, te, tr = s["reward"], s["value"], s["terminated"], s["truncated"]
    done = te | tr
    before = torch.cat([buf.prev_done.bool()[None], done[:-1]])
    adv, ret = torch.empty_like(r), torch.empty_like(r)
    A = torch.zeros(buf.num_envs, dtype=torch.float64, device=r.device)
    nv = last_value.double()
    zero = torch.zeros((), dtype=torch.float64, device=r.device)
    gl = buf.gamma * buf.gae_lambda
    for t in range(T - 1, -1, -1):
        val = v[t].double()
        delta = (r[t].double() + torch.where(te[t], zero, buf.gamma * nv)) - val
        A = torch.where(before[t], zero, delta + torch.where(done[t], zero, gl * A))
        adv[t] = A
        ret[t] = A + val
        nv = val
    valid = ~before
    x = adv.double()
    n = valid.sum()
    mean = torch.where(valid, x, zero).sum() / n
    var = torch.where(valid, (x - mean) ** 2, zero).sum() / n
    norm = torch.where(valid, (x - mean) / torch.sqrt(var + buf.eps), zero).float()
    return adv, ret, valid, norm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()

    import torch

    from sparc_amd import RolloutBuffer, WireEDMEnv, WireEDMVectorEnv, _abi, _lib
    from sparc_amd.rollout import SCAN_UNROLL

    for name, T, N, calls, loops in (("wide", 128, 65536, 500, 3), ("long", 2048, 4096, 500, 1)):
        vec = WireEDMVectorEnv(WireEDMEnv(num_envs=N, device="cuda:0", autoreset=True, reward="progress"))
        buf = RolloutBuffer(vec, T)
        gen = torch.Generator(device="cuda:0").manual_seed(1234)
        for key in ("reward", "value"):
            buf.stored[key].normal_(generator=gen)
        for key in ("terminated", "truncated"):   # an episode every hundred steps or so
            buf.stored[key].copy_(torch.rand((T, N), generator=gen, device="cuda:0") < 0.005)
        last = torch.randn(N, generator=gen, device="cuda:0")

        def finish():
            buf._slot = T
            return buf.finish(last)

        finish()   # from here on prev_done is the rollout's own last done row, call after call
        got = {k: v.clone() for k, v in finish().items()}   # warm-up of both sides, and agreement of what they compute
        adv, ret, valid, norm = torch_loop(buf, last)
        torch.cuda.synchronize()
        worst = max(float((got["advantage"] - adv).abs().max()), float((got["returns"] - ret).abs().max()),
                    float((got["advantage_norm"] - norm).abs().max()))
        assert torch.equal(got["valid"], valid) and worst < 1e-4, worst
        ms = {"device": [], "torch": []}
        for _ in range(args.rounds):
            ms["device"].append(timed(finish, calls))
            ms["torch"].append(timed(lambda: torch_loop(buf, last), loops))
        desc, flags, phases = buf._desc, buf._desc.flags, {}
        for phase, bit in (("scan", _abi.GAE_SCAN), ("apply", _abi.GAE_APPLY)):
            desc.flags = flags | bit
            phases[phase] = [timed(lambda: vec.env._backend.gae(desc), calls) for _ in range(args.rounds)]
        desc.flags = flags
        med = {k: statistics.median(v) for k, v in ms.items()}
        nbytes = T * N * (10 + 9 + 8)
        print(json.dumps({
            "workload": name, "T": T, "num_envs": N, "scan_unroll": SCAN_UNROLL, "device_ms": med["device"], "torch_loop_ms": med["torch"],
            "torch_over_device": med["torch"] / med["device"], "scan_alone_ms": statistics.median(phases["scan"]),
            "apply_alone_ms": statistics.median(phases["apply"]), "algorithmic_bytes": nbytes,
            "achieved_GB_per_s": nbytes / (med["device"] * 1e-3) / 1e9,
            "scan_GB_per_s": T * N * 19 / (statistics.median(phases["scan"]) * 1e-3) / 1e9,
            "largest_difference_to_the_torch_loop": worst, "build_id": _lib.build_id(), "ms": ms, "phase_ms": phases,
        }))
        del vec, buf


if __name__ == "__main__":
    main()
