#!/usr/bin/env python
"""Cost of the optimiser step as `wedm_adam` (through `Adam`) against what torch composes for the same step --
``torch.nn.utils.clip_grad_norm_([theta], max_norm)`` followed by ``torch.optim.AdamW([theta]).step()``, in its ``fused=True``
and its foreach form --, in the same process and build, in alternating rounds, timed with event pairs, medians.

  step      one step over n float32 parameters with clipping on, at n = 1 024 ... 65 536, at 6 418 (`PolicyNet`'s default theta)
            and at 40 732 (the largest `PolicyNet`): the one-block form (no phase bit, n <= WEDM_OPT_ONE_BLOCK_MAX of the loaded
            library), the phased form (all three phase bits in one call: three launches), and torch's two;
  epoch     the epoch of tools/policy_net_cost.py (128 x 65 536 rows in 8 minibatches: ``net(rollout=, index=)``,
            `PPOLoss.backward(rollout=, index=)`, the network's backward into ``theta.grad``) followed in every minibatch by
            ``opt.step(stats)`` with clipping and the KL gate, or by torch's composition without any look at the KL.

The threshold WEDM_OPT_ONE_BLOCK_MAX is chosen from ``step``.  The shipped library runs the one-block form only up to it; for
the one-block times beyond it, build part 0 of the kernels file with ``-DWEDM_OPT_ONE_BLOCK_MAX=65536`` and point WEDM_HIP_LIB
at that library (sparc_amd/_lib.py).

    python tools/optimizer_cost.py [--rounds 7] [--out profiles/r18/optimizer_cost.jsonl] [--no-epoch]

Prints one JSON line per workload (every sample in it) and writes them to ``--out``."""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SIZES = (1024, 2048, 4096, 6418, 8192, 16384, 32768, 40732, 65536)
MAX_NORM = 0.5


def timed(fn, count):
    import torch

    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(count):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / count  # ms per call


def step_lines(args, torch, _abi, _lib, Adam):
    dev = "cuda:0"
    one_max = _abi.OPT_ONE_BLOCK_MAX if args.one_block_max is None else args.one_block_max
    gen = torch.Generator(device=dev).manual_seed(99)
    lines = []
    for n in SIZES:
        theta = torch.randn(n, generator=gen, device=dev).requires_grad_(True)
        theta.grad = torch.randn(n, generator=gen, device=dev) / n ** 0.5
        opt = Adam(theta, lr=3e-4, max_grad_norm=MAX_NORM)
        L = _lib.load()

        def ours(flags):
            d = _abi.OptDesc(theta=theta.data_ptr(), m=opt.m.data_ptr(), v=opt.v.data_ptr(), grad=theta.grad.data_ptr(),
                             partials=opt._partials.data_ptr(), state=opt.state.data_ptr(), info=opt._info.data_ptr(), kl=None,
                             lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-5, weight_decay=0.0, max_norm=MAX_NORM, kl_limit=0.0, n=n,
                             flags=_abi.OPT_CLIP | flags)
            return lambda: _lib.call_stateless(L.wedm_adam, torch.device(dev), C.byref(d))

        leaf = theta.detach().clone().requires_grad_(True)
        leaf.grad = theta.grad.clone()
        fused = torch.optim.AdamW([leaf], lr=3e-4, eps=1e-5, weight_decay=0.0, fused=True)
        foreach = torch.optim.AdamW([leaf], lr=3e-4, eps=1e-5, weight_decay=0.0, foreach=True)

        def torch_step(o):
            def fn():
                torch.nn.utils.clip_grad_norm_([leaf], MAX_NORM)
                o.step()
            return fn

        work = {"phased": ours(_abi.OPT_NORM | _abi.OPT_DECIDE | _abi.OPT_APPLY), "adam_step": opt.step,
                "torch_fused": torch_step(fused), "torch_foreach": torch_step(foreach)}
        if n <= one_max:
            work["one_block"] = ours(0)
        for fn in work.values():   # warm-up: code loaded, torch's state allocated
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in work}
        for _ in range(args.rounds):
            for k, fn in work.items():
                ms[k].append(timed(fn, 300))
        line = {"workload": "step", "n": n, "build_id": _lib.build_id(), "one_block_max": one_max,
                **{f"{k}_us": 1e3 * statistics.median(v) for k, v in ms.items()}, "ms": ms}
        lines.append(line)
        print(json.dumps(line), flush=True)
    return lines


def epoch_lines(args, torch, _lib, Adam):
    from sparc_amd import PolicyHead, PolicyNet, PPOLoss, RolloutBuffer, WireEDMEnv, WireEDMVectorEnv

    dev, N, T, parts, hidden = "cuda:0", 65536, 128, 8, (64, 64)
    TN = T * N
    B = TN // parts
    vec = WireEDMVectorEnv(WireEDMEnv(num_envs=N, device=dev, pulse_stats=True, signal_stats=True))
    head = PolicyHead(vec, modes=(1, 3, 5, 7, 9, 11, 13, 15, 17), seed=1)
    ppo = PPOLoss(head, clip=0.2, vf_coef=0.5, ent_coef=0.01)
    net = PolicyNet(vec, head, hidden=hidden, activation="tanh", seed=1)
    D, M = net.obs_dim, len(head.modes)
    gen = torch.Generator(device=dev).manual_seed(1234)
    # a rollout's blocks: one real step allocates them, seeded values fill them (the time does not depend on the physics)
    buf = RolloutBuffer(vec, T, extras={"log_prob": torch.float32})
    vec.reset(seed=1)
    obs = torch.randn(N, D, generator=gen, device=dev)
    with torch.no_grad():
        out = head.sample(net.forward(obs)[0])
    zero = torch.zeros(N, device=dev)
    buf.add(obs, head.stored(out), zero, zero, zero.bool(), zero.bool(), log_prob=out.log_prob)
    flat = {**{k: v.view((TN,) + tuple(v.shape[2:])) for k, v in buf.stored.items()}, **{k: v.view(TN) for k, v in buf.computed.items()}}
    with torch.no_grad():
        for j in range(parts):
            s = slice(j * B, (j + 1) * B)
            flat["obs"][s] = torch.randn(B, D, generator=gen, device=dev)
            p, _ = net.forward(flat["obs"][s])
            flat["action.u"][s] = p[:, 0:4] + p[:, 4:8].exp() * torch.randn(B, 4, generator=gen, device=dev)
            flat["action.mode_index"][s] = torch.randint(0, M, (B,), generator=gen, device=dev, dtype=torch.int32)
            flat["log_prob"][s] = head.evaluate(p, flat["action.u"][s], flat["action.mode_index"][s])[0]
        flat["value"].copy_(torch.randn(TN, generator=gen, device=dev))
        flat["advantage_norm"].copy_(torch.randn(TN, generator=gen, device=dev))
        flat["returns"].copy_(flat["value"] + torch.randn(TN, generator=gen, device=dev))
        flat["valid"].copy_(torch.rand(TN, generator=gen, device=dev) >= 0.02)
    perm_gen = torch.Generator(device=dev)
    start = net.theta.detach().clone()
    ours = Adam(net, lr=1e-5, max_grad_norm=MAX_NORM, kl_limit=1e9)
    fused = torch.optim.AdamW([net.theta], lr=1e-5, eps=1e-5, weight_decay=0.0, fused=True)
    foreach = torch.optim.AdamW([net.theta], lr=1e-5, eps=1e-5, weight_decay=0.0, foreach=True)

    def epoch(step):
        def fn():
            perm_gen.manual_seed(77)
            with torch.no_grad():
                net.theta.copy_(start)
            ours.begin_update()
            for idx in torch.tensor_split(torch.randperm(TN, device=dev, generator=perm_gen), parts):
                net.theta.grad = None
                params, value = net(rollout=buf, index=idx)
                stats = ppo.backward(params, value, rollout=buf, index=idx)
                step(stats)
        return fn

    def torch_step(o):
        def fn(stats):
            torch.nn.utils.clip_grad_norm_([net.theta], MAX_NORM)
            o.step()
        return fn

    work = {"no_step": epoch(lambda stats: None), "adam": epoch(ours.step), "torch_fused": epoch(torch_step(fused)),
            "torch_foreach": epoch(torch_step(foreach))}
    for fn in work.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in work}
    for _ in range(args.rounds):
        for k, fn in work.items():
            ms[k].append(timed(fn, 2))
    line = {"workload": "epoch", "rows": TN, "minibatches": parts, "n_theta": net.n_theta, "build_id": _lib.build_id(),
            **{f"{k}_ms": statistics.median(v) for k, v in ms.items()}, "ms": ms}
    print(json.dumps(line), flush=True)
    vec.close()
    return [line]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r18" / "optimizer_cost.jsonl"))
    ap.add_argument("--no-epoch", action="store_true")
    ap.add_argument("--one-block-max", type=int, default=None, help="WEDM_OPT_ONE_BLOCK_MAX of the library WEDM_HIP_LIB names")
    args = ap.parse_args()

    import torch

    from sparc_amd import Adam, _abi, _lib

    assert torch.cuda.is_available(), "the cost is a measurement on the MI355X"
    lines = step_lines(args, torch, _abi, _lib, Adam)
    if not args.no_epoch:
        lines += epoch_lines(args, torch, _lib, Adam)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("".join(json.dumps(line) + "\n" for line in lines))


if __name__ == "__main__":
    main()
