"""python tools/minibatch_cost.py [--reps 15] [--warmup 3]

What one shuffled minibatch costs behind a rollout: float32 SB3_FLAT rows (F = 40, 160 bytes), five float32 columns (values,
log-probs, advantages, returns, rewards) and int32 actions, int64 indices cut from a torch.randperm(T * N), at
(T, N, B) = (658, 6, 203) -- the reference's PPO batch on its own env count -- (658, 4 096, 203), (20, 65 536, 65 536) and
(658, 65 536, 65 536), measured in one process, the variants alternating from one repetition to the next:

  minibatch  HipEngine.minibatch() = ptg_minibatch, one kernel, outputs preallocated        HIP events around the call
  torch      the same batch with torch on the same tensors: t, e = idx % T, idx // T, then
             x[t, e] per array (seven advanced-indexing launches), eager                     HIP events around the lines
  copy       obs_out.copy_(the first B rows of the observation buffer): a plain contiguous
             copy of the same B x 160 bytes, the bandwidth yardstick                         HIP events around the call

Every timed section is queued behind a ~100 us device-side delay, so the host has enqueued its work (argument checks, ctypes,
the launches) before the first event is reached: the events bracket device work only -- for the launch-bound torch route the
device then waits for the host inside the interval, which is that route's cost.  Medians with min and max over --reps
repetitions after --warmup unrecorded ones.  Compulsory bytes per gathered row: F * 4 read + F * 4 written + 8 of index +
2 * 4 per column = 376; of the copy: 2 * F * 4 = 320.  GB/s = those bytes / the median time."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cost_timing import stats, timed  # noqa: E402

SHAPES = [(658, 6, 203), (658, 4096, 203), (20, 65536, 65536), (658, 65536, 65536)]
HBM_PEAK = 8.0e12


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

    print(f"# tools/minibatch_cost.py: float32 SB3_FLAT rows (160 B), 5 float32 columns + int32 actions, int64 indices; {args.reps} repetitions "
          f"after {args.warmup} warm-up, variants alternating; device time from HIP events [us]: median [min - max]")
    print(f"# torch {torch.__version__}; {torch.cuda.get_device_name(0)}")
    print(f"{'T':>4s} {'N':>6s} {'B':>6s}  {'minibatch':>26s}  {'torch route':>29s}  {'copy of B rows':>26s}  {'bytes':>10s} {'GB/s':>7s} {'of 8 TB/s':>9s} "
          f"{'copy GB/s':>9s} {'torch/mb':>8s} {'mb/copy':>7s}")
    for T, n, B in SHAPES:
        eng = HipEngine(spec.consts, spec.tables, spec.markets, n, device=0, out_dtype="float32", obs_layout="sb3_flat")
        eng.set_episode_plan(spec.eps_ind, n, n)
        eng.set_noise_rng(11)
        eng.reset()
        F = eng.obs_dim
        g = torch.Generator(device="cuda")
        g.manual_seed(T + n)
        acts = torch.randint(0, 5, (T, n), dtype=torch.int32, device=dev, generator=g)
        obs, rew, _ = eng.rollout(acts)                       # real observation rows
        cols = [torch.randn((T, n), dtype=torch.float32, device=dev, generator=g) for _ in range(4)] + [rew, acts]
        idx = torch.randperm(T * n, device=dev, generator=g)[:B].contiguous()
        assert idx.shape[0] == B and idx.dtype == torch.int64
        out = torch.empty((B, F), dtype=torch.float32, device=dev)
        outs = [torch.empty((B,), dtype=c.dtype, device=dev) for c in cols]
        out_c = torch.empty((B, F), dtype=torch.float32, device=dev)
        flat = obs.view(T * n, F)

        def torch_route():
            t, e = idx % T, idx // T
            return obs[t, e], [c[t, e] for c in cols]

        times = {"mb": [], "torch": [], "copy": []}
        for rep in range(args.warmup + args.reps):
            t_m, _ = timed(lambda: eng.minibatch(idx, obs, cols, obs_out=out, columns_out=outs))
            t_t, (o_t, c_t) = timed(torch_route)
            t_c, _ = timed(lambda: out_c.copy_(flat[:B]))
            if rep >= args.warmup:
                times["mb"].append(t_m); times["torch"].append(t_t); times["copy"].append(t_c)
        eng.sync()
        same = torch.equal(out.view(torch.int32), o_t.view(torch.int32)) and all(
            torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(outs, c_t))
        assert same, "the torch route and ptg_minibatch disagree"
        nbytes = B * (2 * F * 4 + 8 + 2 * 4 * len(cols))
        med = {k: statistics.median(v) for k, v in times.items()}
        fmt = lambda k: stats(times[k])
        gbs = nbytes / (med["mb"] * 1e-6) / 1e9
        gbs_c = B * 2 * F * 4 / (med["copy"] * 1e-6) / 1e9
        print(f"{T:4d} {n:6d} {B:6d}  {fmt('mb'):>26s}  {fmt('torch'):>29s}  {fmt('copy'):>26s}  {nbytes:10d} {gbs:7.1f} {gbs * 1e9 / HBM_PEAK:9.4f} "
              f"{gbs_c:9.1f} {med['torch'] / med['mb']:8.2f} {med['mb'] / med['copy']:7.2f}   # torch route byte-equal: {same}")
        eng.close()
        del obs, rew, cols, acts, flat, out, outs, out_c, o_t, c_t
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
