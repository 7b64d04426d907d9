"""python tools/actor_cost.py [--reps 15] [--warmup 3] [--out profiles/actor_cost.txt]

What the actor half of an off-policy gradient step costs on the device: float32 network outputs, measured in one process, the two
routes alternating from one repetition to the next on the same tensors:

  kernel  HipEngine.rsample (+ rsample_backward) / HipEngine.actor_loss into preallocated outputs and workspace
  torch   the eager route a caller writes today: SB3's lines in float32 -- Actor.action_log_prob (clamp, exp, rsample with torch's
          generator, tanh, Normal.log_prob, the tanh correction) on leaf mean / log_std tensors, backward to .grad from given
          incoming gradients; the SAC / TQC / TD3 actor loss with the entropy-coefficient loss on leaf Q / quantile / log-prob /
          log_ent_coef tensors, forward and backward to .grad

Shapes: rsample forward and forward + backward at B = 470 (SAC's batch) and 65 536; actor_loss at B = 470, K = 2 (SAC), at B = 290,
K = 2, Q = 30 (TQC), at B = 257, K = 1 (TD3) and at B = 65 536 (SAC).
Every timed section is queued behind a ~100 us device-side delay, so the host has enqueued its work before the first event is
reached: the events bracket device work only -- for the launch-bound torch route the device then waits for the host inside the
interval, which is that route's cost.  Medians with min and max over --reps repetitions after --warmup unrecorded ones.
Compulsory bytes per row at float32: rsample forward 8 read, 8 + 8 (the float64 noise) written = 24; forward + backward 24 + 8 + 8
(the noise again) + 8 read and 8 written = 56; SAC's loss, K = 2: 8 + 4 read, 8 + 4 written = 24; TQC's, K = 2, Q = 30: 240 + 4 read,
240 + 4 written = 488; TD3's: 4 read, 4 written.  The floor of the small shapes is one short launch between two events (6-7 us,
profiles/minibatch_cost.txt), two for a loss beyond 256 rows, plus the counter kernel behind a stochastic rsample."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cost_timing  # noqa: E402
from cost_timing import stats  # noqa: E402

RS_SHAPES = [470, 65536]
AL_SHAPES = [("sac", 470, 2, 1), ("tqc", 290, 2, 30), ("td3", 257, 1, 1), ("sac", 65536, 2, 1)]
H_T = -1.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "actor_cost.txt"))
    args = ap.parse_args()
    import torch
    from rl_ptg_amd import dist as ptg_dist
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    spec, _ = synthetic_spec(scenario=1, operation="OP1", eps_len_d=32)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    eng = HipEngine(spec.consts, spec.tables, spec.markets, 6, device=0, out_dtype="float32", obs_layout="sb3_flat")      # the reference's 6 envs; B is not tied to it
    first_ptr, stride = ptg_dist.episode_plan(6, 1, 0)
    eng.set_episode_plan(spec.eps_ind, first_ptr, stride)

    def torch_action_log_prob(mean, log_std, ga, gl, backward):
        def run():
            mean.grad = None; log_std.grad = None
            ls = torch.clamp(log_std, -20, 2)
            action_std = torch.ones_like(mean) * ls.exp()
            dist = torch.distributions.Normal(mean, action_std)
            gaussian_actions = dist.rsample()
            actions = torch.tanh(gaussian_actions)
            log_prob = dist.log_prob(gaussian_actions).sum(dim=1)
            log_prob = log_prob - torch.sum(torch.log(1 - actions ** 2 + 1e-6), dim=1)
            if backward:
                torch.autograd.backward([actions, log_prob], [ga, gl])
            return actions, log_prob
        return run

    def torch_actor(kind, qs, lp, log_ent_coef):
        def run():
            for x in qs + [lp, log_ent_coef]:
                x.grad = None
            if kind == "td3":
                actor_loss = -qs[0].mean()
                actor_loss.backward()
                return actor_loss
            log_prob = lp.reshape(-1, 1)
            ent_coef = torch.exp(log_ent_coef.detach())
            ent_coef_loss = -(log_ent_coef * (log_prob + H_T).detach()).mean()
            ent_coef_loss.backward()
            if kind == "sac":
                q_values_pi = torch.cat(qs, dim=1)
                min_qf_pi, _ = torch.min(q_values_pi, dim=1, keepdim=True)
                actor_loss = (ent_coef * log_prob - min_qf_pi).mean()
            else:
                qf_pi = qs[0].mean(dim=2).mean(dim=1, keepdim=True)
                actor_loss = (ent_coef * log_prob - qf_pi).mean()
            actor_loss.backward()
            return actor_loss
        return run

    say(f"# tools/actor_cost.py: float32 means, log_stds, Q-values, quantiles and log-probs; {args.reps} repetitions after {args.warmup} warm-up, routes alternating; "
        f"device time from HIP events [us]: median [min - max]")
    say(f"# torch {torch.__version__}; {torch.cuda.get_device_name(0)}; library {os.environ.get('PTG_LIB_PATH', 'in-tree default')}")
    say(f"{'op':>22s} {'B':>7s} {'launches':>8s}  {'kernel route':>30s}  {'torch route':>30s} {'torch/kernel':>12s}  {'GB/s':>7s}")
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    rnd = lambda *shape: torch.rand(shape, device=dev, generator=g)

    def row(name, B, launches, tk, tt, nbytes):
        mk, mt = statistics.median(tk), statistics.median(tt)
        say(f"{name:>22s} {B:7d} {launches:8d}  {stats(tk):>30s}  {stats(tt):>30s} {mt / mk:12.2f}  {B * nbytes / mk * 1e-3:7.1f}")
        if min(tt) <= max(tk):
            say(f"#   the two ranges overlap: kernel max {max(tk):.1f} us, torch min {min(tt):.1f} us")
        if mk > mt:
            say(f"#   THE KERNEL ROUTE'S MEDIAN IS ABOVE THE TORCH ROUTE'S: {mk:.1f} against {mt:.1f} us")

    counter = eng.new_draw_counter()
    for B in RS_SHAPES:
        mean = (rnd(B, 1) * 2 - 1).requires_grad_(True)
        log_std = (rnd(B, 1) * 2.5 - 3).requires_grad_(True)
        ga, gl = rnd(B, 1) * 2 - 1, rnd(B) * 2 - 1
        res = eng.rsample(mean.detach(), log_std.detach(), counter)
        grads = eng.rsample_backward(mean.detach(), log_std.detach(), res.noise, ga, gl)
        fwd = lambda: eng.rsample(mean.detach(), log_std.detach(), counter, out=res)

        def both():
            eng.rsample(mean.detach(), log_std.detach(), counter, out=res)
            eng.rsample_backward(mean.detach(), log_std.detach(), res.noise, ga, gl, out=grads)

        tk, tt = cost_timing.alternate(fwd, torch_action_log_prob(mean, log_std, ga, gl, False), args.warmup, args.reps)
        row("rsample forward", B, 2, tk, tt, 24)
        tk, tt = cost_timing.alternate(both, torch_action_log_prob(mean, log_std, ga, gl, True), args.warmup, args.reps)
        row("rsample fwd + bwd", B, 3, tk, tt, 56)
        eng.sync()
    for kind, B, K, Q in AL_SHAPES:
        lp = (rnd(B) * 5 - 4).requires_grad_(True)
        log_alpha = torch.tensor([-1.3125], dtype=torch.float64, device=dev)
        la32 = log_alpha.float().requires_grad_(True)
        ws = eng.actor_loss_workspace(B)
        if kind == "tqc":
            qs = [(rnd(B, K, Q) * 16 - 8).requires_grad_(True)]
            call = lambda out=None: eng.actor_loss("tqc", qs[0].detach(), lp.detach(), log_ent_coef=log_alpha, target_entropy=H_T, out=out, workspace=ws)
            nbytes = 8 * K * Q + 8
        elif kind == "sac":
            qs = [(rnd(B, 1) * 16 - 8).requires_grad_(True) for _ in range(K)]
            call = lambda out=None: eng.actor_loss("sac", [x.detach() for x in qs], lp.detach(), log_ent_coef=log_alpha, target_entropy=H_T, out=out, workspace=ws)
            nbytes = 8 * K + 8
        else:
            qs = [(rnd(B, 1) * 16 - 8).requires_grad_(True)]
            call = lambda out=None: eng.actor_loss("td3", qs[0].detach(), out=out, workspace=ws)
            nbytes = 8
        route = torch_actor(kind, qs, lp, la32)
        res = call()
        tk, tt = cost_timing.alternate(lambda: call(res), route, args.warmup, args.reps)
        eng.sync()
        ref = route()
        torch.cuda.synchronize()
        gq = res.grad_q if isinstance(res.grad_q, list) else [res.grad_q]
        n = B * K * Q
        diff = max(float((a - b.grad).abs().max()) for a, b in zip(gq, qs)) * n
        row(f"actor_loss {kind} K={K} Q={Q}", B, 1 if B <= 256 else 2, tk, tt, nbytes)
        say(f"#   actor loss: kernel {float(res.stats[0]):.7f}, torch {float(ref.detach()):.7f}; max |d loss / d q difference| x B K Q: {diff:.2e}")
    say("# GB/s: compulsory bytes per row (see the module docstring) over the kernel route's median; it means something for the 65 536-row shapes only -- the")
    say("# reference's batch sizes are bound by launch latency.  The torch route computes in float32 and draws with torch's generator, the kernel route in")
    say("# float64 rounded once with the counter RNG: the two rsample routes draw different noise, so only the losses are set side by side.")
    say("# not measured: float64 inputs, K and Q other than those above, lists of per-critic quantile tensors, strided inputs and gradients, a host or")
    say("# device-scalar alpha, the deterministic call, TD3's smoothed target action, the entropy-coefficient loss alone, the captured (hipGraph) calls,")
    say("# rl_ptg_amd.loss's autograd wrappers (a contiguous copy and a multiply per tensor in backward), the host time of a call, the kernels under a profiler.")
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
