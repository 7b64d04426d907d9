"""python tools/sde_cost.py [--reps 15] [--warmup 3] [--out profiles/sde_cost.txt]

What gSDE (SB3's use_sde, the reference's `gSDE : True`) costs on the device for the on-policy algorithms: float32 network outputs,
measured in one process, the two routes alternating from one repetition to the next on the same tensors:

  kernel  HipEngine.sde_resample / sde_act / sde_policy_loss into preallocated outputs and workspace
  torch   the eager route a caller writes today: SB3's StateDependentNoiseDistribution lines in float32 -- sample_weights
          (Normal(0, exp(log_std)).rsample((N,))); proba_distribution (mm of the squared latent and the squared std, sqrt), sample (bmm),
          clamp, log_prob, entropy; evaluate_actions and the loss lines of PPO.train / A2C.train on leaf mean / values / log_std
          tensors (learn_features=False: the latent is data), forward and backward to .grad

Shapes: the head and the matrix at N = 6 (the reference's envs), 4 096 and 65 536 with L = 358 (PPO's last hidden layer) and 808 (A2C's);
the loss at B = 203, L = 358 (PPO's minibatch), B = 3 948, L = 808 (A2C's one batch of 658 x 6) and B = 65 536, L = 358, with and
without the latent gradient.
Every timed section is queued behind a ~100 us device-side delay, so the host has enqueued its work before the first event is
reached: the events bracket device work only -- for the launch-bound torch route the device then waits for the host inside the
interval, which is that route's cost.  Medians with min and max over --reps repetitions after --warmup unrecorded ones.
Compulsory bytes per row at float32 (s = 4): the head 2 L s (the latent and the matrix) + 4 + 4 + 12 (mean, action, raw / log-prob /
entropy); the matrix L s written; the loss L s (the latent) + 24 (mean, value, sample, old log-prob, advantage, return) + 8 (two
gradients), and L s more written with the latent gradient."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cost_timing  # noqa: E402
from cost_timing import stats  # noqa: E402

HEAD_SHAPES = [(6, 358), (6, 808), (4096, 358), (4096, 808), (65536, 358), (65536, 808)]
LOSS_SHAPES = [("ppo", 203, 358), ("a2c", 3948, 808), ("ppo", 65536, 358)]
CLIP, ENT_COEF, VF_COEF = 0.2, 0.01, 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sde_cost.txt"))
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
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

    def engine(n):
        eng = HipEngine(spec.consts, spec.tables, spec.markets, n, device=0, out_dtype="float32", obs_layout="sb3_flat")
        first_ptr, stride = ptg_dist.episode_plan(n, 1, 0)
        eng.set_episode_plan(spec.eps_ind, first_ptr, stride)
        return eng

    say(f"# tools/sde_cost.py: float32 means, values, latents and log_std; {args.reps} repetitions after {args.warmup} warm-up, routes alternating; "
        f"device time from HIP events [us]: median [min - max]")
    say(f"# torch {torch.__version__}; {torch.cuda.get_device_name(0)}; library {os.environ.get('PTG_LIB_PATH', 'in-tree default')}")
    say(f"{'op':>22s} {'rows':>7s} {'L':>5s} {'launches':>8s}  {'kernel route':>30s}  {'torch route':>30s} {'torch/kernel':>12s}  {'GB/s':>7s} {'of 8 TB/s':>9s}")
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    rnd = lambda *shape: torch.rand(shape, device=dev, generator=g)
    missed = []

    def row(name, rows, L, launches, tk, tt, nbytes):
        mk, mt = statistics.median(tk), statistics.median(tt)
        gbs = rows * nbytes / mk * 1e-3
        say(f"{name:>22s} {rows:7d} {L:5d} {launches:8d}  {stats(tk):>30s}  {stats(tt):>30s} {mt / mk:12.2f}  {gbs:7.1f} {gbs / 8000 * 100:8.2f}%")
        if min(tt) <= max(tk):
            say(f"#   the two ranges overlap: kernel max {max(tk):.1f} us, torch min {min(tt):.1f} us")
        if mk > mt:
            missed.append(f"{name} rows={rows} L={L}")
            say(f"#   THE KERNEL ROUTE'S MEDIAN IS ABOVE THE TORCH ROUTE'S: {mk:.1f} against {mt:.1f} us")

    engs = {}
    for N, L in HEAD_SHAPES:
        eng = engs.get(N) or engs.setdefault(N, engine(N))
        mean, latent, log_std = rnd(N) * 2 - 1, torch.tanh(rnd(N, L) * 4 - 2), rnd(L) * 2 - 3
        counter, E = eng.new_draw_counter(), torch.zeros(N, L, device=dev)
        out = eng.sde_act_outputs(torch.float32)
        ls2 = log_std.reshape(L, 1)
        state = {}

        def torch_weights():
            std = torch.exp(ls2)
            weights_dist = torch.distributions.Normal(torch.zeros_like(std), std)
            state["E"] = weights_dist.rsample((N,))          # [N, L, 1]
            return state["E"]

        def torch_head():
            std = torch.exp(ls2)
            variance = torch.mm(latent ** 2, std ** 2)
            dist = torch.distributions.Normal(mean.reshape(-1, 1), torch.sqrt(variance + 1e-6))
            noise = torch.bmm(latent.unsqueeze(dim=1), state["E"]).squeeze(dim=1)
            actions = dist.mean + noise
            log_prob = dist.log_prob(actions).sum(dim=1)
            entropy = dist.entropy().sum(dim=1)
            return torch.clamp(actions, -1.0, 1.0), actions, log_prob, entropy

        torch_weights()
        tk, tt = cost_timing.alternate(lambda: eng.sde_resample(log_std, counter, E, seed=1), torch_weights, args.warmup, args.reps)
        row("sde_resample", N, L, 2, tk, tt, 4 * L)
        draws = N * L / statistics.median(tk)
        say(f"#   {draws:.0f} double-precision Box-Muller draws (hash chain, log, sqrt, cos, one product) per us")
        tk, tt = cost_timing.alternate(lambda: eng.sde_act(mean, latent, log_std, E, out=out), torch_head, args.warmup, args.reps)
        row("sde_act", N, L, 1, tk, tt, 8 * L + 20)
        eng.sync()
    eng = engs[6]                                            # B is not tied to the engine's envs
    for kind, B, L in LOSS_SHAPES:
        ppo = kind == "ppo"
        latent, log_std = torch.tanh(rnd(B, L) * 4 - 2), (rnd(L) * 2 - 3).requires_grad_(True)
        mean, values = (rnd(B) * 2 - 1).requires_grad_(True), (rnd(B) * 2 - 1).requires_grad_(True)
        with torch.no_grad():
            sd = torch.sqrt(torch.mm(latent ** 2, torch.exp(log_std.reshape(L, 1)) ** 2) + 1e-6).reshape(-1)
            actions = mean + sd * (rnd(B) * 4 - 2)
            old_lp = torch.distributions.Normal(mean, sd).log_prob(actions) - (rnd(B) - 0.5)
        adv, ret = rnd(B) * 4 - 2, rnd(B) * 2 - 1
        ws = eng.sde_policy_loss_workspace(B, L)

        def torch_loss():
            for x in (mean, values, log_std):
                x.grad = None
            std = torch.exp(log_std.reshape(L, 1))
            variance = torch.mm(latent ** 2, std ** 2)
            dist = torch.distributions.Normal(mean.reshape(-1, 1), torch.sqrt(variance + 1e-6))
            log_prob = dist.log_prob(actions.reshape(-1, 1)).sum(dim=1)
            entropy = dist.entropy().sum(dim=1)
            advantages = adv
            if ppo:
                advantages = (advantages - advantages.mean()) / (advantages.std() + 1e-8)
                ratio = torch.exp(log_prob - old_lp)
                policy_loss = -torch.min(advantages * ratio, advantages * torch.clamp(ratio, 1 - CLIP, 1 + CLIP)).mean()
            else:
                policy_loss = -(advantages * log_prob).mean()
            value_loss = F.mse_loss(ret, values)
            loss = policy_loss + ENT_COEF * (-torch.mean(entropy)) + VF_COEF * value_loss
            loss.backward()
            return loss

        def call(out=None, lat_grad=False):
            return eng.sde_policy_loss(kind, mean.detach(), values.detach(), latent, log_std.detach(), actions, old_lp if ppo else None, adv, ret,
                                       clip_range=CLIP if ppo else None, ent_coef=ENT_COEF, vf_coef=VF_COEF, want_grad_latent=lat_grad, out=out, workspace=ws)

        launches = 4 + (2 if ppo and B > 1 else 0)
        for lat_grad in (False, True):
            res = call(lat_grad=lat_grad)
            tk, tt = cost_timing.alternate(lambda: call(res), torch_loss, args.warmup, args.reps)
            row(f"sde_policy_loss {kind}" + (" +dh" if lat_grad else ""), B, L, launches, tk, tt, 4 * L * (2 if lat_grad else 1) + 32)
        eng.sync()
        ref = torch_loss()
        torch.cuda.synchronize()
        say(f"#   loss: kernel {float(res.stats[0]):.7f}, torch {float(ref.detach()):.7f}; max |d loss / d log_std difference| x B: "
            f"{float((res.grad_log_std - log_std.grad).abs().max()) * B:.2e}; the torch route has no latent gradient (learn_features=False) in either row")
    say("# GB/s: compulsory bytes per row (see the module docstring) over the kernel route's median, and its share of the 8 TB/s HBM peak; it means")
    say("# something for the 65 536-row shapes only -- the reference's sizes are bound by launch latency.  The torch route computes in float32 and draws")
    say("# with torch's generator, the kernel route in float64 rounded once with the counter RNG: the two matrices differ, so only the losses are set side by side.")
    say("# the condition: at every shape the kernel route's median is not above the torch route's -- " + ("met" if not missed else "MISSED at " + "; ".join(missed)))
    say("# not measured: float64 inputs, strided inputs, the deterministic head, the captured (hipGraph) calls, rl_ptg_amd.loss's autograd wrappers,")
    say("# the host time of a call, the kernels under a profiler.")
    for e in engs.values():
        e.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
