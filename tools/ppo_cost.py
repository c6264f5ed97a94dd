#!/usr/bin/env python
"""Cost of PPO's loss as one call (wedm_ppo_loss through `PPOLoss`) against the path a user had before it, in the same
process and build, in alternating rounds, timed with event pairs, medians.  One epoch is 128 x 65 536 rows in 8 minibatches
of 1 048 576 at M = 9 modes; the parameter rows and value estimates of a minibatch are leaves that stand for a network's
output (the network, and gathering its observations, are the same on every path and are not timed):

  a  `PPOLoss.backward` on the minibatch's stored tensors, already gathered;
  b  `PPOLoss.backward(rollout=, index=)`: the buffer's blocks read in place, the ``randperm`` and its split included;
  c  today's path: `RolloutBuffer.minibatches` (a ``randperm`` and an index-select of every block), `PolicyHead.evaluate`,
     the clipped surrogate, value loss and entropy bonus in torch weighted by ``valid``, ``backward()``;
  c0 the same without `minibatches`: the stored tensors already gathered, as in a.

Before timing, a and c0 are asserted to agree on the gradient to float32's accuracy.  Also times MAIN by itself on one
minibatch at M = 1, 9 and 19 modes next to the head's EVALUATE and BACKWARD.

    python tools/ppo_cost.py [--rounds 5] [--out profiles/r4/ppo_cost.jsonl]

Prints one JSON line per workload (every sample in it) and writes them to ``--out``."""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

CLIP, VF_COEF, ENT_COEF = 0.2, 0.5, 0.01


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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r4" / "ppo_cost.jsonl"))
    args = ap.parse_args()

    import torch

    from sparc_amd import PolicyHead, PPOLoss, RolloutBuffer, WireEDMEnv, WireEDMVectorEnv, _abi, _lib
    from sparc_amd.policy_head import BACKWARD, EVALUATE
    from sparc_amd.ppo import device_ppo_loss

    dev, N, T, parts = "cuda:0", 65536, 128, 8
    B, TN = T * N // parts, T * N
    vec = WireEDMVectorEnv(WireEDMEnv(num_envs=N, device=dev))
    head = PolicyHead(vec, modes=(1, 3, 5, 7, 9, 11, 13, 15, 17), seed=1)
    ppo = PPOLoss(head, clip=CLIP, vf_coef=VF_COEF, ent_coef=ENT_COEF)
    P, M = head.param_dim, len(head.modes)
    gen = torch.Generator(device=dev).manual_seed(1234)

    def rows(n, P=P):
        p = torch.randn(n, P, generator=gen, device=dev)
        p[:, 4:8] = p[:, 4:8].clamp(-2.0, 1.0) - 1.0
        return p

    # ---- a rollout's blocks: one real step allocates them, seeded values fill them (the time does not depend on the physics)
    buf = RolloutBuffer(vec, T, extras={"log_prob": torch.float32})
    obs, _ = vec.reset(seed=1)
    out = head.sample(rows(N))
    zero = torch.zeros(N, device=dev)
    buf.add(obs, head.stored(out), zero, zero, zero.bool(), zero.bool(), log_prob=out.log_prob)
    flat = {**{k: v.view((TN,) + tuple(v.shape[2:])) for k, v in buf.stored.items()},
            **{k: v.view(TN) for k, v in buf.computed.items()}}
    current = torch.empty(TN, P, device=dev)   # the policy's rows at every stored step, a little off the sampling policy
    with torch.no_grad():
        for j in range(parts):
            s = slice(j * B, (j + 1) * B)
            p = rows(B)
            flat["action.u"][s] = p[:, 0:4] + p[:, 4:8].exp() * torch.randn(B, 4, generator=gen, device=dev)
            flat["action.mode_index"][s] = torch.randint(0, M, (B,), generator=gen, device=dev, dtype=torch.int32)
            flat["log_prob"][s] = head.evaluate(p, flat["action.u"][s], flat["action.mode_index"][s])[0]
            current[s] = p + 0.05 * torch.randn(B, P, generator=gen, device=dev)
        flat["value"].copy_(torch.randn(TN, generator=gen, device=dev))
        flat["advantage_norm"].copy_(torch.randn(TN, generator=gen, device=dev))
        flat["returns"].copy_(flat["value"] + torch.randn(TN, generator=gen, device=dev))
        flat["valid"].copy_(torch.rand(TN, generator=gen, device=dev) >= 0.02)
        now_value = flat["value"] + 0.3 * torch.randn(TN, generator=gen, device=dev)
    buf_flat = buf.flat()
    stored_names = dict(u="action.u", mode_index="action.mode_index", old_log_prob="log_prob", advantage="advantage_norm",
                        returns="returns", valid="valid")

    perm_gen = torch.Generator(device=dev)

    def permutation():
        perm_gen.manual_seed(77)   # the same permutation every epoch: the leaves below belong to its minibatches
        return torch.randperm(TN, device=dev, generator=perm_gen)

    leaf = lambda t: t.clone().requires_grad_(True)   # noqa: E731
    dense = [(leaf(current[j * B:(j + 1) * B]), leaf(now_value[j * B:(j + 1) * B]),
              {k: buf_flat[name][j * B:(j + 1) * B] for k, name in stored_names.items()}) for j in range(parts)]
    shuffled = [(leaf(current[idx]), leaf(now_value[idx])) for idx in torch.tensor_split(permutation(), parts)]
    del current, now_value

    def epoch_a():
        for p, v, s in dense:
            p.grad = v.grad = None
            ppo.backward(p, v, **s)

    def epoch_b():
        for (p, v), idx in zip(shuffled, torch.tensor_split(permutation(), parts)):
            p.grad = v.grad = None
            ppo.backward(p, v, rollout=buf, index=idx)

    def torch_loss(p, v, s):
        lp, ent = head.evaluate(p, s["u"], s["mode_index"])
        w = s["valid"].to(torch.float32)
        n = w.sum()
        ratio = torch.exp(lp - s["old_log_prob"])
        adv = s["advantage"]
        policy = -(torch.minimum(ratio * adv, ratio.clamp(1.0 - CLIP, 1.0 + CLIP) * adv) * w).sum() / n
        value = 0.5 * (((v - s["returns"]) ** 2) * w).sum() / n
        entropy = (ent * w).sum() / n
        return policy + VF_COEF * value - ENT_COEF * entropy

    def epoch_c():
        perm_gen.manual_seed(77)
        for (p, v), mb in zip(shuffled, buf.minibatches(parts, generator=perm_gen)):
            p.grad = v.grad = None
            torch_loss(p, v, {k: mb[name] for k, name in stored_names.items()}).backward()

    def epoch_c0():
        for p, v, s in dense:
            p.grad = v.grad = None
            torch_loss(p, v, s).backward()

    epochs = {"a": (epoch_a, 20), "b": (epoch_b, 10), "c": (epoch_c, 5), "c0": (epoch_c0, 10)}
    for fn, _ in epochs.values():   # warm-up: buffers grown, code loaded
        fn()
    epoch_a()
    got = (dense[0][0].grad.clone(), dense[0][1].grad.clone())
    epoch_c0()
    torch.cuda.synchronize()
    want = (dense[0][0].grad, dense[0][1].grad)
    worst = max(float(((g - w).abs() / (1e-12 + w.abs().max())).max()) for g, w in zip(got, want))
    assert worst < 1e-3, worst
    ms = {k: [] for k in epochs}
    for _ in range(args.rounds):
        for k, (fn, count) in epochs.items():
            ms[k].append(timed(fn, count))
    med = {k: statistics.median(v) for k, v in ms.items()}
    lines = [{"workload": "epoch", "rows": TN, "minibatches": parts, "modes": M, "a_backward_gathered_ms": med["a"],
              "b_backward_rollout_index_ms": med["b"], "c_today_minibatches_evaluate_torch_ms": med["c"],
              "c0_today_gathered_ms": med["c0"], "c0_over_a": med["c0"] / med["a"], "c_over_b": med["c"] / med["b"],
              "largest_gradient_difference_relative_to_the_largest_gradient": worst, "build_id": _lib.build_id(), "ms": ms}]
    print(json.dumps(lines[-1]), flush=True)
    del dense, shuffled, got, want

    # ---- MAIN by itself next to the head's two launches, by the number of modes
    for m in (1, 9, 19):
        p_dim = 8 + m
        p = rows(B, p_dim)
        u = (p[:, 0:4] + p[:, 4:8].exp() * torch.randn(B, 4, generator=gen, device=dev)).contiguous()
        k = torch.randint(0, m, (B,), generator=gen, device=dev, dtype=torch.int32)
        g = torch.randn(5, B, generator=gen, device=dev)
        lp, ent, grad, gv = torch.empty(B, device=dev), torch.empty(B, device=dev), torch.empty(B, p_dim, device=dev), torch.empty(B, device=dev)
        d = head._desc(EVALUATE, B)   # (the descriptor takes any mode numbers and count; `PolicyHead` only crater modes)
        d.n_modes, d.param_stride, d.grad_stride = m, p_dim, p_dim
        d.modes[:m] = list(range(1, m + 1))
        d.params, d.u, d.mode_index, d.log_prob, d.entropy = p.data_ptr(), u.data_ptr(), k.data_ptr(), lp.data_ptr(), ent.data_ptr()
        d.g_log_prob, d.g_entropy, d.grad_params = g[0].data_ptr(), g[1].data_ptr(), grad.data_ptr()
        phases = {}
        for name, op in (("evaluate", EVALUATE), ("backward", BACKWARD)):
            d.op = op
            vec.env._backend.policy_head(d)
        torch.cuda.synchronize()
        old = (lp + 0.1 * g[4]).contiguous()
        q = _abi.PpoDesc(params=p.data_ptr(), value=g[2].data_ptr(), u=u.data_ptr(), mode_index=k.data_ptr(), old_log_prob=old.data_ptr(),
                         advantage=g[0].data_ptr(), returns=g[3].data_ptr(), grad_params=grad.data_ptr(), grad_value=gv.data_ptr(),
                         partials=ppo._partials.data_ptr(), stats=ppo._stats.data_ptr(), param_stride=p_dim, grad_stride=p_dim,
                         n_src=B, clip=CLIP, vf_coef=VF_COEF, ent_coef=ENT_COEF, n_modes=m, rows=B, flags=_abi.PPO_MAIN)
        q.lo[:], q.hi[:], q.log_span[:] = head._lo, head._hi, head._log_span
        device_ppo_loss(q, dev)
        phases = {"evaluate": [], "backward": [], "main": []}
        for _ in range(args.rounds):
            for name, op in (("evaluate", EVALUATE), ("backward", BACKWARD)):
                d.op = op
                phases[name].append(timed(lambda: vec.env._backend.policy_head(d), 200))
            phases["main"].append(timed(lambda: device_ppo_loss(q, dev), 200))
        ev, bw, mn = (statistics.median(phases[name]) for name in ("evaluate", "backward", "main"))
        lines.append({"workload": "launches", "rows": B, "modes": m, "evaluate_ms": ev, "backward_ms": bw, "main_ms": mn,
                      "main_over_evaluate_plus_backward": mn / (ev + bw), "main_ns_per_row": mn * 1e6 / B,
                      "build_id": _lib.build_id(), "phase_ms": phases})
        print(json.dumps(lines[-1]), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("".join(json.dumps(line) + "\n" for line in lines))


if __name__ == "__main__":
    main()
