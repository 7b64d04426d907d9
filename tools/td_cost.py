"""python tools/td_cost.py [--reps 15] [--warmup 3] [--out profiles/td_cost.txt]

What the TD loss of a replay batch and its gradients cost on the device: float32 Q-values, float32 rewards and dones (what
DeviceReplayBuffer.sample() of a float32 engine returns), measured in one process, the two routes alternating from one repetition
to the next on the same tensors:

  ptg_td_loss  HipEngine.td_loss into preallocated outputs and workspace: one kernel up to 256 rows; rows + final merge beyond
  torch        the eager route a caller writes today: SB3's lines (the target under no_grad -- th.max / th.min, SAC's entropy term,
               (1 - dones) * gamma -- gather + smooth_l1_loss for DQN, the sum of mse_loss for the critics) on leaf Q tensors with
               requires_grad, forward and backward to .grad

Shapes: DQN (A = 5, the reference's discrete action space, int64 actions as the replay buffer keeps them) at B = 544 (the
reference's batch) and 65 536; TD3 (K = 2 critics) at 257; SAC (K = 2, log alpha in a device scalar) at 470 and 65 536.
Every timed section is queued behind a ~100 us device-side delay, so the host has enqueued its work before the first event is
reached: the events bracket device work only -- for the launch-bound torch route the device then waits for the host inside the
interval, which is that route's cost.  Medians with min and max over --reps repetitions after --warmup unrecorded ones.
Compulsory bytes per row at float32: DQN 20 + 20 (Q and next-Q rows) + 8 (action) + 8 (reward, done) read and 20 written = 76;
critics, K = 2: 8 + 8 + 8 read and 8 written = 32, SAC 4 more for the log-prob.  The floor of the small shapes is one short launch
between two events (6-7 us, profiles/minibatch_cost.txt)."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cost_timing  # noqa: E402
from cost_timing import stats  # noqa: E402

A, K = 5, 2
GAMMA = {"dqn": 0.9728, "td3": 0.9595, "sac": 0.9628}      # config/config_agent.yaml of the reference
SHAPES = [("dqn", 544), ("dqn", 65536), ("td3", 257), ("sac", 470), ("sac", 65536)]
BYTES = {"dqn": 76, "td3": 32, "sac": 36}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "td_cost.txt"))
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

    eng = HipEngine(spec.consts, spec.tables, spec.markets, 6, device=0, out_dtype="float32", obs_layout="sb3_flat")      # the reference's 6 envs; B is not tied to it
    first_ptr, stride = ptg_dist.episode_plan(6, 1, 0)
    eng.set_episode_plan(spec.eps_ind, first_ptr, stride)

    def torch_dqn(q, next_q, actions, rewards, dones, gamma):
        def run():
            q.grad = None
            with torch.no_grad():
                next_q_values, _ = next_q.max(dim=1)
                next_q_values = next_q_values.reshape(-1, 1)
                target_q_values = rewards + (1 - dones) * gamma * next_q_values
            current_q_values = torch.gather(q, dim=1, index=actions)
            loss = F.smooth_l1_loss(current_q_values, target_q_values)
            loss.backward()
            return loss
        return run

    def torch_critics(kind, qs, next_qs, rewards, dones, gamma, next_log_prob, log_ent_coef):
        def run():
            for x in qs:
                x.grad = None
            with torch.no_grad():
                next_q_values = torch.cat(next_qs, dim=1)
                next_q_values, _ = torch.min(next_q_values, dim=1, keepdim=True)
                if kind == "sac":
                    ent_coef = torch.exp(log_ent_coef.detach())
                    next_q_values = next_q_values - ent_coef * next_log_prob.reshape(-1, 1)
                target_q_values = rewards + (1 - dones) * gamma * next_q_values
            critic_loss = sum(F.mse_loss(current_q, target_q_values) for current_q in qs)
            if kind == "sac":
                critic_loss = 0.5 * critic_loss
            critic_loss.backward()
            return critic_loss
        return run

    say(f"# tools/td_cost.py: float32 Q-values, rewards and dones; DQN A = {A}, int64 actions; critics K = {K}; {args.reps} repetitions after {args.warmup} warm-up, "
        f"routes alternating; device time from HIP events [us]: median [min - max]")
    say(f"# torch {torch.__version__}; {torch.cuda.get_device_name(0)}; library {os.environ.get('PTG_LIB_PATH', 'in-tree default')}")
    say(f"{'loss':>6s} {'B':>7s} {'launches':>8s}  {'ptg_td_loss':>30s}  {'torch route':>30s} {'torch/kernel':>12s}  {'GB/s':>7s}")
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    rnd = lambda *shape: torch.rand(shape, device=dev, generator=g)
    for kind, B in SHAPES:
        gamma = GAMMA[kind]
        rewards, dones = rnd(B, 1) * 6 - 3, (rnd(B, 1) < 0.1).float()
        ws = eng.td_loss_workspace(B)
        if kind == "dqn":
            q = (rnd(B, A) * 16 - 8).requires_grad_(True)
            next_q = rnd(B, A) * 16 - 8
            actions = torch.randint(0, A, (B, 1), device=dev, generator=g)
            call = lambda out=None: eng.td_loss("dqn", q.detach(), next_q, rewards, dones, gamma, actions=actions, out=out, workspace=ws)
            route = torch_dqn(q, next_q, actions, rewards, dones, gamma)
            leaves = [q]
        else:
            qs = [(rnd(B, 1) * 16 - 8).requires_grad_(True) for _ in range(K)]
            next_qs = [rnd(B, 1) * 16 - 8 for _ in range(K)]
            lp = rnd(B) * 5 - 4
            log_alpha = torch.tensor([-1.3125], dtype=torch.float64, device=dev)
            kw = dict(next_log_prob=lp, log_ent_coef=log_alpha) if kind == "sac" else {}
            call = lambda out=None: eng.td_loss(kind, [x.detach() for x in qs], next_qs, rewards, dones, gamma, out=out, workspace=ws, **kw)
            route = torch_critics(kind, qs, next_qs, rewards, dones, gamma, lp, log_alpha.float())
            leaves = qs
        res = call()
        tk, tt = cost_timing.alternate(lambda: call(res), route, args.warmup, args.reps)
        eng.sync()
        ref = route()
        torch.cuda.synchronize()
        grads = [res.grad_q] if kind == "dqn" else res.grad_q
        diff = max(float((a - b.grad).abs().max()) for a, b in zip(grads, leaves)) * B
        say(f"{kind:>6s} {B:7d} {1 if B <= 256 else 2:8d}  {stats(tk):>30s}  {stats(tt):>30s} {statistics.median(tt) / statistics.median(tk):12.2f}  "
            f"{B * BYTES[kind] / statistics.median(tk) * 1e-3:7.1f}")
        say(f"#   loss: kernel {float(res.stats[0]):.7f}, torch {float(ref.detach()):.7f}; max |grad difference| x B: {diff:.2e}")
    say("# GB/s: compulsory bytes (76 per row DQN, 32 TD3, 36 SAC) over the kernel route's median; it means something for the 65 536-row shapes only -- the")
    say("# reference's batch sizes are bound by launch latency.  The torch route computes in float32, the kernel in float64 rounded once: hence the differences above.")
    say("# not measured: float64 inputs, A other than 5, K other than 2, strided inputs and gradients, a host alpha, the target output (want_target), the captured")
    say("# (hipGraph) call, rl_ptg_amd.loss's autograd wrappers (one more copy and a multiply per critic in backward), the kernels under a profiler.")
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
