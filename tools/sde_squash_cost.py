"""python tools/sde_squash_cost.py [--reps 15] [--warmup 3] [--out profiles/sde_squash_cost.txt]

What gSDE (SB3's use_sde, the reference's `gSDE : True`) costs on the device for SAC and TQC: float32 network outputs, measured in
one process, the two routes alternating from one repetition to the next on the same tensors:

  kernel  HipEngine.sde_resample_rows / sde_rsample / sde_rsample_backward into preallocated outputs and workspace
  torch   the eager route a caller writes today: SB3's StateDependentNoiseDistribution lines in float32 as sac/policies.py::Actor uses
          them -- reset_noise() (Normal(0, exp(log_std)).rsample()), F.hardtanh, proba_distribution (mm, sqrt), get_noise (mm for the
          shared row, bmm while collecting), tanh, log_prob with the atanh round trip and the log(1 - a^2 + 1e-6) correction; forward
          and backward of (ent_coef * log_prob - w * a).mean() to the .grad of leaf mean / latent / log_std tensors

Shapes: the forward + backward pair and the no-grad forward at SAC's 470 x 233 and TQC's 290 x 708 (batch x the trunk's width); the
collecting head at 6 (the reference's envs), 4 096 and 65 536 envs x 233 / 708; sde_resample_rows at 1 row.
Every timed section is queued behind a ~100 us device-side delay (tools/cost_timing.py), so the events bracket device work only -- for
the launch-bound torch route the device then waits for the host inside the interval, which is that route's cost.  Medians with min and
max over --reps repetitions after --warmup unrecorded ones.
Compulsory bytes per row at float32 (s = 4): the shared-row forward L s (the latent) + 4 + 8 (mean, action, log-prob) + 16 (saved); the
backward L s (the latent) + L s (its gradient) + 4 + 8 + 4 + 16; the collecting head 2 L s (the latent and the matrix row) + 4 + 8
(mean, the action in both forms)."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cost_timing  # noqa: E402
from cost_timing import stats  # noqa: E402

TRAIN_SHAPES = [("SAC", 470, 233), ("TQC", 290, 708)]
HEAD_SHAPES = [(6, 233), (6, 708), (4096, 233), (4096, 708), (65536, 233), (65536, 708)]
CLIP_MEAN, ENT_COEF = 2.0, 0.2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sde_squash_cost.txt"))
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from rl_ptg_amd import dist as ptg_dist
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    spec, _ = synthetic_spec(scenario=1, operation="OP1", eps_len_d=32, action_type="continuous")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def engine(n):
        eng = HipEngine(spec.consts, spec.tables, spec.markets, n, device=0, out_dtype="float32", obs_layout="sb3_flat")
        first_ptr, stride = ptg_dist.episode_plan(n, 1, 0)
        eng.set_episode_plan(spec.eps_ind, first_ptr, stride)
        return eng

    say(f"# tools/sde_squash_cost.py: float32 means, latents and log_std; {args.reps} repetitions after {args.warmup} warm-up, routes alternating; "
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
        verdict = "held" if mk <= mt else "MISSED"
        say(f"{name:>22s} {rows:7d} {L:5d} {launches:8d}  {stats(tk):>30s}  {stats(tt):>30s} {mt / mk:12.2f}  {gbs:7.1f} {gbs / 8000 * 100:8.2f}%  {verdict}")
        if min(tt) <= max(tk):
            say(f"#   the two ranges overlap: kernel max {max(tk):.1f} us, torch min {min(tt):.1f} us")
        if mk > mt:
            missed.append(f"{name} rows={rows} L={L}")
            say(f"#   THE KERNEL ROUTE'S MEDIAN IS ABOVE THE TORCH ROUTE'S: {mk:.1f} against {mt:.1f} us")

    def sb3_lines(mean, latent, log_std, E, shared):
        """SB3's lines from the unclipped mean to (actions, log_prob); E: [L, 1] (mm) or [N, L, 1] (bmm)"""
        std = torch.exp(log_std)
        mean_actions = F.hardtanh(mean, -CLIP_MEAN, CLIP_MEAN)
        variance = torch.mm(latent ** 2, std ** 2)
        dist = torch.distributions.Normal(mean_actions, torch.sqrt(variance + 1e-6))
        noise = torch.mm(latent, E) if shared else torch.bmm(latent.unsqueeze(dim=1), E).squeeze(dim=1)
        actions = torch.tanh(dist.mean + noise)
        eps = torch.finfo(actions.dtype).eps
        y = actions.clamp(min=-1.0 + eps, max=1.0 - eps)
        gaussian_actions = 0.5 * (y.log1p() - (-y).log1p())
        log_prob = dist.log_prob(gaussian_actions).sum(dim=-1)
        log_prob = log_prob - torch.sum(torch.log(1.0 - actions ** 2 + 1e-6), dim=1)
        return actions, log_prob

    eng = engine(6)                                          # B is not tied to the engine's envs
    for algo, B, L in TRAIN_SHAPES:
        mean, latent = (rnd(B, 1) * 5 - 2.5).requires_grad_(True), torch.tanh(rnd(B, L) * 4 - 2).requires_grad_(True)
        log_std = (rnd(L, 1) * 2 - 3).requires_grad_(True)
        w = rnd(B) * 2 - 1
        counter, E = eng.new_draw_counter(), torch.zeros(L, device=dev)
        state = {}

        def torch_reset():
            std = torch.exp(log_std)
            state["E"] = torch.distributions.Normal(torch.zeros_like(std), std).rsample()      # [L, 1], with its path into log_std
            return state["E"]

        def torch_pair():
            for x in (mean, latent, log_std):
                x.grad = None
            torch_reset()
            actions, log_prob = sb3_lines(mean, latent, log_std, state["E"], True)
            loss = (ENT_COEF * log_prob - w * actions[:, 0]).mean()
            loss.backward()
            return loss

        def torch_target():
            with torch.no_grad():
                return sb3_lines(mean, latent, log_std, state["E"], True)

        tk, tt = cost_timing.alternate(lambda: eng.sde_resample_rows(log_std.detach(), counter, E, seed=1), torch_reset, args.warmup, args.reps)
        row(f"{algo} resample_rows", 1, L, 2, tk, tt, 4 * L)
        m, h, ls = mean.detach(), latent.detach(), log_std.detach()
        ga, gl = (-w / B).contiguous(), torch.full((B,), ENT_COEF / B, device=dev)
        fo = eng.sde_rsample(m, h, ls, E)
        bo = eng.sde_rsample_backward(m, h, ls, E, fo.saved, ga, gl)
        ws = eng.sde_rsample_backward_workspace(B, L)

        def kernel_pair():
            eng.sde_resample_rows(ls, counter, E, seed=1)
            f = eng.sde_rsample(m, h, ls, E, out=fo)
            return eng.sde_rsample_backward(m, h, ls, E, f.saved, ga, gl, out=bo, workspace=ws)

        tk, tt = cost_timing.alternate(kernel_pair, torch_pair, args.warmup, args.reps)
        row(f"{algo} reset + fwd + bwd", B, L, 6, tk, tt, 8 * L + 32 + 12 + 16)
        fn = eng.sde_rsample(m, h, ls, E, want_saved=False)
        tk, tt = cost_timing.alternate(lambda: eng.sde_rsample(m, h, ls, E, out=fn), torch_target, args.warmup, args.reps)
        row(f"{algo} no-grad forward", B, L, 1, tk, tt, 4 * L + 12)
        eng.sync()
    engs = {6: eng}
    for N, L in HEAD_SHAPES:
        e = engs.get(N) or engs.setdefault(N, engine(N))
        mean, latent, log_std = rnd(N, 1) * 5 - 2.5, torch.tanh(rnd(N, L) * 4 - 2), rnd(L, 1) * 2 - 3
        counter, E = e.new_draw_counter(), torch.zeros(N, L, device=dev)
        e.sde_resample(log_std, counter, E, seed=1)
        std = torch.exp(log_std)
        E3 = torch.distributions.Normal(torch.zeros_like(std), std).rsample((N,))                 # [N, L, 1]
        out = e.sde_rsample(mean, latent, log_std, E, want_step_actions=True, want_logp=False, want_saved=False)

        def torch_head():
            with torch.no_grad():
                std = torch.exp(log_std)
                mean_actions = F.hardtanh(mean, -CLIP_MEAN, CLIP_MEAN)
                noise = torch.bmm(latent.unsqueeze(dim=1), E3).squeeze(dim=1)
                return torch.tanh(mean_actions + noise), std                                       # sample() alone: no log-prob while collecting

        tk, tt = cost_timing.alternate(lambda: e.sde_rsample(mean, latent, log_std, E, out=out), torch_head, args.warmup, args.reps)
        row("collecting head", N, L, 1, tk, tt, 8 * L + 12)
        e.sync()
    say("# GB/s: compulsory bytes per row (see the module docstring) over the kernel route's median, and its share of the 8 TB/s HBM peak; it means")
    say("# something for the 65 536-row shapes only -- the reference's sizes are bound by launch latency.  The torch route computes in float32 and draws")
    say("# with torch's generator, the kernel route in float64 rounded once with the counter RNG.  The kernel route's collecting head also forms the variance")
    say("# (its saved pair and log-prob are switched off, the sum stays); the torch route's collecting head is sample() alone.")
    say("# the condition: at every shape the kernel route's median is not above the torch route's -- " + ("held at every shape" if not missed else "MISSED at " + "; ".join(missed)))
    say("# not measured: float64 inputs, strided inputs, the deterministic head, the captured (hipGraph) calls, rl_ptg_amd.loss's autograd wrapper,")
    say("# SquashedSdeNoise's own overhead, the host time of a call, the kernels under a profiler.")
    for e in engs.values():
        e.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
