"""python tools/loss_cost.py [--reps 15] [--warmup 3] [--out profiles/loss_cost.txt]

What the loss of a minibatch and its gradients cost on the device: float32, A = 5 (the reference's discrete action space), measured
in one process, the two routes alternating from one repetition to the next on the same tensors:

  ptg_policy_loss  HipEngine.policy_loss into preallocated outputs and workspace: one kernel up to 256 rows; rows + final merge
                   beyond, with two more kernels in front for the advantage moments when they are normalised
  torch            the eager route a caller writes today: SB3's lines (Categorical / Normal log_prob and entropy, the loss lines of
                   PPO.train / A2C.train) on leaf logits / values with requires_grad, forward and backward to .grad

Shapes: B = 203 (the reference's PPO minibatch), 4 096 and 20 x 65 536 (an A2C window); PPO with advantage normalisation (no value
clipping: SB3's default) and A2C without; the Gaussian head at B = 203.
Every timed section is queued behind a ~100 us device-side delay, so the host has enqueued its work before the first event is
reached: the events bracket device work only -- for the launch-bound torch route the device then waits for the host inside the
interval, which is that route's cost.  Medians with min and max over --reps repetitions after --warmup unrecorded ones.
Compulsory bytes per row at float32, A = 5, int32 actions: 20 (logits) + 4 (value) + 4 (action) + 12 (old log-prob, advantage,
return) read and 24 written = 64 (PPO; A2C 60), plus 4 more read where the advantages are normalised (they are read twice) --
84 MB for the A2C window; the floor of the small shapes is one short launch between two events (6-7 us,
profiles/minibatch_cost.txt)."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cost_timing  # noqa: E402
from cost_timing import stats  # noqa: E402

BS = [203, 4096, 20 * 65536]
A = 5
CLIP, ENT_COEF, VF_COEF = 0.2, 0.01, 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "loss_cost.txt"))
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from torch.distributions import Categorical, Normal
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

    alternate = lambda fa, fb: cost_timing.alternate(fa, fb, args.warmup, args.reps)

    eng = HipEngine(spec.consts, spec.tables, spec.markets, 6, device=0, out_dtype="float32", obs_layout="sb3_flat")      # the reference's 6 envs; B is not tied to it
    first_ptr, stride = ptg_dist.episode_plan(6, 1, 0)
    eng.set_episode_plan(spec.eps_ind, first_ptr, stride)

    def torch_route(kind, x, values, actions, old_lp, adv, ret, log_std=None):
        def run():
            x.grad = None; values.grad = None
            if log_std is not None:
                log_std.grad = None
                d = Normal(x, torch.ones_like(x) * log_std.exp(), validate_args=False)
            else:
                d = Categorical(logits=x, validate_args=False)
            log_prob, entropy = d.log_prob(actions), d.entropy()
            advantages = adv
            if kind == "ppo":
                advantages = (advantages - advantages.mean()) / (advantages.std() + 1e-8)
                ratio = torch.exp(log_prob - old_lp)
                policy_loss = -torch.min(advantages * ratio, advantages * torch.clamp(ratio, 1 - CLIP, 1 + CLIP)).mean()
                clip_fraction = torch.mean((torch.abs(ratio - 1) > CLIP).float())
                with torch.no_grad():
                    log_ratio = log_prob - old_lp
                    approx_kl = torch.mean((torch.exp(log_ratio) - 1) - log_ratio)
            else:
                policy_loss = -(advantages * log_prob).mean()
                clip_fraction = approx_kl = None
            loss = policy_loss + ENT_COEF * -torch.mean(entropy) + VF_COEF * F.mse_loss(ret, values)
            loss.backward()
            return loss, clip_fraction, approx_kl
        return run

    say(f"# tools/loss_cost.py: float32, A = {A}, int32 actions; {args.reps} repetitions after {args.warmup} warm-up, routes alternating; "
        f"device time from HIP events [us]: median [min - max]")
    say(f"# torch {torch.__version__}; {torch.cuda.get_device_name(0)}; library {os.environ.get('PTG_LIB_PATH', 'in-tree default')}")
    say(f"{'loss':>14s} {'B':>8s}  {'ptg_policy_loss':>30s}  {'torch route':>30s} {'torch/kernel':>12s}  {'GB/s':>7s}")
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    for B in BS:
        x = (torch.randn((B, A), device=dev, generator=g) * 3).requires_grad_(True)
        values = torch.randn(B, device=dev, generator=g).requires_grad_(True)
        actions = torch.randint(0, A, (B,), dtype=torch.int32, device=dev, generator=g)
        act64 = actions.long()
        with torch.no_grad():
            old_lp = Categorical(logits=x).log_prob(act64) - (torch.rand(B, device=dev, generator=g) - 0.5)
        adv, ret = torch.randn(B, device=dev, generator=g), torch.randn(B, device=dev, generator=g)
        ws = eng.policy_loss_workspace(B)
        for kind, nbytes in (("ppo", 68), ("a2c", 60)):
            kw = dict(clip_range=CLIP) if kind == "ppo" else {}
            call = lambda out=None: eng.policy_loss(kind, x.detach(), values.detach(), actions, old_lp if kind == "ppo" else None, adv, ret, ent_coef=ENT_COEF,
                                                    vf_coef=VF_COEF, out=out, workspace=ws, **kw)
            res = call()
            tk, tt = alternate(lambda: call(res), torch_route(kind, x, values, act64, old_lp, adv, ret))
            eng.sync()
            ref = torch_route(kind, x, values, act64, old_lp, adv, ret)()
            torch.cuda.synchronize()
            say(f"{kind + ' categorical':>14s} {B:8d}  {stats(tk):>30s}  {stats(tt):>30s} {statistics.median(tt) / statistics.median(tk):12.2f}  "
                f"{B * nbytes / statistics.median(tk) * 1e-3:7.1f}")
            say(f"#   loss: kernel {float(res.stats[0]):.7f}, torch {float(ref[0]):.7f}; max |grad difference| x B: logits "
                f"{float((res.grad_input - x.grad).abs().max()) * B:.2e}, values {float((res.grad_values - values.grad).abs().max()) * B:.2e}")
    B = 203
    mean = (torch.randn(B, device=dev, generator=g) * 0.5).requires_grad_(True)
    values = torch.randn(B, device=dev, generator=g).requires_grad_(True)
    log_std = torch.full((1,), -0.7, device=dev).requires_grad_(True)
    with torch.no_grad():
        raw = mean + log_std.exp() * torch.randn(B, device=dev, generator=g)
        old_lp = Normal(mean, log_std.exp()).log_prob(raw) - (torch.rand(B, device=dev, generator=g) - 0.5)
    adv, ret = torch.randn(B, device=dev, generator=g), torch.randn(B, device=dev, generator=g)
    ws = eng.policy_loss_workspace(B)
    call = lambda out=None: eng.policy_loss("ppo", mean.detach(), values.detach(), raw, old_lp, adv, ret, clip_range=CLIP, ent_coef=ENT_COEF, vf_coef=VF_COEF,
                                            log_std=log_std.detach(), out=out, workspace=ws)
    res = call()
    tk, tt = alternate(lambda: call(res), torch_route("ppo", mean, values, raw, old_lp, adv, ret, log_std))
    eng.sync()
    say(f"{'ppo gaussian':>14s} {B:8d}  {stats(tk):>30s}  {stats(tt):>30s} {statistics.median(tt) / statistics.median(tk):12.2f}  {B * 48 / statistics.median(tk) * 1e-3:7.1f}")
    say(f"#   max |grad difference| x B: means {float((res.grad_input - mean.grad).abs().max()) * B:.2e}, log_std {float((res.grad_log_std - log_std.grad).abs().max()):.2e}")
    say("# GB/s: compulsory bytes (68 per row PPO with normalisation, 60 A2C, 48 Gaussian PPO) over the kernel route's median; it means something for the")
    say("# 20 x 65 536 window only -- the smaller shapes are bound by launch latency.")
    say("# not measured: float64 inputs, A other than 5, int64 actions, strided [B, A + 1] inputs and gradients, value clipping, the captured (hipGraph)")
    say("# call, rl_ptg_amd.loss's autograd wrapper (one more copy and two multiplies in backward), the kernels under a profiler, B between 4 096 and 20 x 65 536.")
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
