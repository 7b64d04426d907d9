"""python tools/quantile_cost.py [--reps 15] [--warmup 3] [--out profiles/quantile_cost.txt]

What TQC's quantile-Huber critic loss of a replay batch and its gradients cost on the device: float32 quantiles, float32 rewards and
dones (what DeviceReplayBuffer.sample() of a float32 engine returns), K = 2 critics of Q = 30 quantiles, d = 2 dropped per net (the
reference's TQC), log alpha in a device scalar, measured in one process, the two routes alternating from one repetition to the next
on the same tensors:

  ptg_quantile_loss  HipEngine.quantile_loss into preallocated outputs and workspace: one wave per row, four rows per workgroup; one
                     kernel up to 4 rows, rows + final merge beyond
  torch              the eager route a caller writes today: sb3_contrib's lines (th.sort, the slice, the entropy term and
                     (1 - dones) * gamma under no_grad; quantile_huber_loss(sum_over_quantiles=False) with its [B, K, Q, M] pairwise
                     tensor) on a leaf [B, K, Q] tensor with requires_grad, forward and backward to .grad

Shapes: B = 290 (the reference's batch), 65 536, and 4 (the one-launch route).
Every timed section is queued behind a ~100 us device-side delay, so the host has enqueued its work before the first event is
reached: the events bracket device work only -- for the launch-bound torch route the device then waits for the host inside the
interval, which is that route's cost.  Medians with min and max over --reps repetitions after --warmup unrecorded ones.
Compulsory bytes per row at float32: 240 + 240 (current and next quantiles) + 12 (reward, done, log-prob) read and 240 written = 732.
The floor of the small shapes is two short launches between two events (~10 us, profiles/td_cost.txt)."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cost_timing  # noqa: E402
from cost_timing import stats  # noqa: E402

K, Q, DROP = 2, 30, 2
GAMMA = 0.9639                                            # config/config_agent.yaml of the reference
SHAPES = [290, 65536, 4]
BYTES = 4 * (3 * K * Q + 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "quantile_cost.txt"))
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
    n_target_quantiles = K * Q - DROP * K

    def torch_tqc(current_quantiles, next_quantiles_in, rewards, dones, gamma, next_log_prob, log_ent_coef):
        def run():
            current_quantiles.grad = None
            with torch.no_grad():
                ent_coef = torch.exp(log_ent_coef.detach())
                batch_size = next_quantiles_in.shape[0]
                next_quantiles, _ = torch.sort(next_quantiles_in.reshape(batch_size, -1))
                next_quantiles = next_quantiles[:, :n_target_quantiles]
                target_quantiles = next_quantiles - ent_coef * next_log_prob.reshape(-1, 1)
                target_quantiles = rewards + (1 - dones) * gamma * target_quantiles
                target_quantiles.unsqueeze_(dim=1)
            # quantile_huber_loss(current_quantiles, target_quantiles, sum_over_quantiles=False)
            n_quantiles = current_quantiles.shape[-1]
            cum_prob = (torch.arange(n_quantiles, device=current_quantiles.device, dtype=torch.float) + 0.5) / n_quantiles
            cum_prob = cum_prob.view(1, 1, -1, 1)
            pairwise_delta = target_quantiles.unsqueeze(-2) - current_quantiles.unsqueeze(-1)
            abs_pairwise_delta = torch.abs(pairwise_delta)
            huber_loss = torch.where(abs_pairwise_delta > 1, abs_pairwise_delta - 0.5, pairwise_delta ** 2 * 0.5)
            loss = torch.abs(cum_prob - (pairwise_delta.detach() < 0).float()) * huber_loss
            loss = loss.mean()
            loss.backward()
            return loss
        return run

    say(f"# tools/quantile_cost.py: float32 quantiles, rewards and dones; K = {K} critics, Q = {Q} quantiles, d = {DROP} dropped per net (M = {n_target_quantiles}); "
        f"log alpha on the device; {args.reps} repetitions after {args.warmup} warm-up, routes alternating; device time from HIP events [us]: median [min - max]")
    say(f"# torch {torch.__version__}; {torch.cuda.get_device_name(0)}; library {os.environ.get('PTG_LIB_PATH', 'in-tree default')}")
    say(f"{'B':>7s} {'launches':>8s} {'pairs':>11s}  {'ptg_quantile_loss':>30s}  {'torch route':>30s} {'torch/kernel':>12s}  {'GB/s':>7s}")
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    rnd = lambda *shape: torch.rand(shape, device=dev, generator=g)
    for B in SHAPES:
        rewards, dones = rnd(B, 1) * 6 - 3, (rnd(B, 1) < 0.1).float()
        ws = eng.quantile_loss_workspace(B)
        cur = (rnd(B, K, Q) * 6 - 3).requires_grad_(True)
        nxt = rnd(B, K, Q) * 6 - 3
        lp = rnd(B) * 5 - 4
        log_alpha = torch.tensor([-1.3125], dtype=torch.float64, device=dev)
        call = lambda out=None: eng.quantile_loss(cur.detach(), nxt, rewards, dones, lp, GAMMA, DROP, log_ent_coef=log_alpha, out=out, workspace=ws)
        route = torch_tqc(cur, nxt, rewards, dones, GAMMA, lp, log_alpha.float())
        res = call()
        tk, tt = cost_timing.alternate(lambda: call(res), route, args.warmup, args.reps)
        eng.sync()
        ref = route()
        torch.cuda.synchronize()
        n = B * K * Q * n_target_quantiles
        diff = float((res.grad_quantiles - cur.grad).abs().max()) * n
        say(f"{B:7d} {1 if B <= 4 else 2:8d} {n:11d}  {stats(tk):>30s}  {stats(tt):>30s} {statistics.median(tt) / statistics.median(tk):12.2f}  "
            f"{B * BYTES / statistics.median(tk) * 1e-3:7.1f}")
        say(f"#   loss: kernel {float(res.stats[0]):.7f}, torch {float(ref.detach()):.7f}; max |grad difference| x n: {diff:.2e}")
    say(f"# GB/s: compulsory bytes ({BYTES} per row) over the kernel route's median; it means something for the 65 536-row shape only -- the reference's batch is")
    say("# bound by launch latency.  The torch route computes in float32 (cum_prob too), the kernel in float64 rounded once: hence the differences above.")
    say("# not measured: float64 inputs, K, Q and d other than the reference's, lists of per-critic tensors, strided inputs and gradients, a host alpha, the target")
    say("# output (want_target), the captured (hipGraph) call, rl_ptg_amd.loss's autograd wrapper (one more multiply in backward), the kernels under a profiler.")
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
