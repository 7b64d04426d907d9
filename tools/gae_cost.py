"""python tools/gae_cost.py [--reps 15] [--warmup 3]

What generalised advantage estimation costs behind a rollout, float32, at (T, N) = (658, 6) -- the reference's own A2C shape --
(658, 4 096), (20, 65 536) and (658, 65 536), measured in one process, the variants alternating from one repetition to the next:

  gae      HipEngine.gae() = ptg_gae, one kernel                                            HIP events around the call
  torch    SB3's RolloutBuffer.compute_returns_and_advantage, its lines on the same device
           tensors: a Python loop backwards over T, eager launches                           HIP events around the loop
  rollout  HipEngine.rollout() of the same (T, N) from a fresh reset, the fused env kernel  HIP events around the call
           that produced such a window (row-major float32 observations)

Every timed section is queued behind a ~100 us device-side delay, so the host has enqueued its work (argument checks, ctypes,
the launch) before the first event is reached: the events bracket device work only, not host latency on an idle stream -- for the
launch-bound torch loop the device then waits for the host inside the interval, which is that loop's cost.
Medians with min and max over --reps repetitions after --warmup unrecorded ones.  Compulsory bytes of gae: 9 read (reward, value,
done flag) + 8 written (advantage, return) per element, + 4 per env for the last value; GB/s = those bytes / the median time."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cost_timing import stats, timed  # noqa: E402

SHAPES = [(658, 6), (658, 4096), (20, 65536), (658, 65536)]
GAMMA, LAMBDA = 0.9393, 0.9819          # the reference's A2C pair (config/config_agent.yaml)
HBM_PEAK = 8.0e12


def torch_gae(rewards, values, episode_starts, last_values, dones, gamma, gae_lambda, advantages):
    """SB3 2.0.0a13's loop on device tensors"""
    buffer_size = rewards.shape[0]
    last_gae_lam = 0
    for step in reversed(range(buffer_size)):
        if step == buffer_size - 1:
            next_non_terminal = 1.0 - dones
            next_values = last_values
        else:
            next_non_terminal = 1.0 - episode_starts[step + 1]
            next_values = values[step + 1]
        delta = rewards[step] + gamma * next_values * next_non_terminal - values[step]
        last_gae_lam = delta + gamma * gae_lambda * next_non_terminal * last_gae_lam
        advantages[step] = last_gae_lam
    return advantages, advantages + values


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    spec, _ = synthetic_spec(scenario=2, operation="OP2", eps_len_d=32)          # 4 608-step episodes: no boundary inside a window

    print(f"# tools/gae_cost.py: float32, gamma {GAMMA}, gae_lambda {LAMBDA}; {args.reps} repetitions after {args.warmup} warm-up, variants "
          f"alternating; device time from HIP events [us]: median [min - max]")
    print(f"# torch {torch.__version__}; {torch.cuda.get_device_name(0)}")
    print(f"{'T':>4s} {'N':>6s}  {'gae':>26s}  {'torch loop':>32s}  {'rollout':>29s}  {'bytes':>11s} {'GB/s':>7s} {'of 8 TB/s':>9s} {'torch/gae':>9s} {'gae/rollout':>11s}")
    for T, n in SHAPES:
        eng = HipEngine(spec.consts, spec.tables, spec.markets, n, device=0, out_dtype="float32", obs_layout="row")
        eng.set_episode_plan(spec.eps_ind, n, n)
        eng.set_noise_rng(11)
        eng.reset()
        g = torch.Generator(device="cuda")
        g.manual_seed(T + n)
        acts = torch.randint(0, 5, (T, n), dtype=torch.int32, device=dev, generator=g)
        obs = eng.alloc_obs(T)
        rew = torch.empty((T, n), dtype=torch.float32, device=dev)
        done = torch.empty((T, n), dtype=torch.uint8, device=dev)
        eng.rollout(acts, obs, rew, done)
        done = (torch.rand((T, n), device=dev, generator=g) < 0.01).to(torch.uint8)      # staggered episode ends for the arithmetic
        values = torch.randn((T, n), dtype=torch.float32, device=dev, generator=g)
        last_values = torch.randn((n,), dtype=torch.float32, device=dev, generator=g)
        episode_starts = torch.zeros((T, n), dtype=torch.float32, device=dev)
        episode_starts[1:] = done[:-1].float()
        dones = done[-1].float()
        adv, ret = torch.empty_like(rew), torch.empty_like(rew)
        adv_t = torch.empty_like(rew)
        scratch = torch.empty((T, n), dtype=torch.uint8, device=dev)
        times = {"gae": [], "torch": [], "rollout": []}
        for rep in range(args.warmup + args.reps):
            keep = rep >= args.warmup
            t_g, _ = timed(lambda: eng.gae(rew, values, done, last_values, GAMMA, LAMBDA, adv=adv, ret=ret))
            t_t, (_, ret_t) = timed(lambda: torch_gae(rew, values, episode_starts, last_values, dones, GAMMA, LAMBDA, adv_t))
            eng.reset()
            eng.sync()
            t_r, _ = timed(lambda: eng.rollout(acts, obs, rew, scratch))
            if keep:
                times["gae"].append(t_g); times["torch"].append(t_t); times["rollout"].append(t_r)
        eng.gae(rew, values, done, last_values, GAMMA, LAMBDA, adv=adv, ret=ret)          # the last rollout's rewards: compare the two once
        _, ret_t = torch_gae(rew, values, episode_starts, last_values, dones, GAMMA, LAMBDA, adv_t)
        torch.cuda.synchronize()
        assert torch.allclose(adv, adv_t, rtol=1e-5, atol=1e-5) and torch.allclose(ret, ret_t, rtol=1e-5, atol=1e-5)
        same = torch.equal(adv, adv_t) and torch.equal(ret, ret_t)
        nbytes = T * n * 17 + 4 * n
        med = {k: statistics.median(v) for k, v in times.items()}
        fmt = lambda k: stats(times[k])
        gbs = nbytes / (med["gae"] * 1e-6) / 1e9
        print(f"{T:4d} {n:6d}  {fmt('gae'):>26s}  {fmt('torch'):>32s}  {fmt('rollout'):>29s}  {nbytes:11d} {gbs:7.1f} {gbs * 1e9 / HBM_PEAK:9.3f} "
              f"{med['torch'] / med['gae']:9.1f} {med['gae'] / med['rollout']:11.3f}   # torch loop bit-equal: {same}")
        eng.close()
        del obs, rew, done, values, adv, ret, adv_t, episode_starts, scratch
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
