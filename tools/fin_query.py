"""python tools/fin_query.py [--envs 65536] [--reps 25] [--warmup 5]

What the two ways out of the finished-episode ring cost at an episode boundary where every env finishes on one step (a synchronised
batch), measured in one process, the variants alternating from one episode end to the next:

  a       HipEngine.finished_episodes(): the host query (device synchronise, three arrays to the host)              wall clock
  b       finished_episodes_dev() + episode_stats_dev(): the drain and Monitor's statistic, device to device        HIP events around
          the enqueued kernels (b_dev), and wall clock from the first enqueue to the end of a stream synchronise (b_wall)
  c_host  a + dist.all_gather_finished() of the host lists on the nccl backend, one rank                             wall clock
  c_dev   drain + dist.all_gather_finished_dev() of the block on the nccl backend, one rank                          wall clock

Before every timed section the batch is stepped to its episode end and the device is synchronised, so the host query's synchronise
waits for nothing: a is the floor of that route.  Medians with min and max over --reps repetitions after --warmup unrecorded ones."""
import argparse
import os
import socket
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-nccl", action="store_true", help="skip the c legs (no process group)")
    args = ap.parse_args()
    import torch
    import torch.distributed as dist
    from rl_ptg_amd import dist as ptg_dist
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    variants = ["a", "b"]
    if not args.no_nccl:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if "MASTER_PORT" not in os.environ:
            with socket.socket() as s:
                s.bind(("127.0.0.1", 0))
                os.environ["MASTER_PORT"] = str(s.getsockname()[1])
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
        variants += ["c_host", "c_dev"]
    n = args.envs
    spec, _ = synthetic_spec(scenario=2, operation="OP2", eps_len_d=4, sim_step=3600)       # 96-step episodes: the 91st call terminates
    eng = HipEngine(spec.consts, spec.tables, spec.markets, n, device=0, out_dtype="float32", obs_layout="row")
    eng.set_episode_plan(spec.eps_ind, n, n)
    eng.set_noise_rng(11)
    eng.reset()
    T = 13
    obs, rew, done = eng.alloc_obs(T), torch.empty((T, n), dtype=eng.out_dtype, device=dev), torch.empty((T, n), dtype=torch.uint8, device=dev)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    acts = torch.randint(0, 5, (T, n), dtype=torch.int32, device=dev, generator=g)

    def to_episode_end():
        left = eng.steps_to_episode_end()
        while left > 0:
            t = min(T, left)
            eng.rollout(acts[:t], obs[:t], rew[:t], done[:t])
            left -= t
        eng.sync()

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {k: [] for k in ("a", "b_dev", "b_wall", "c_host", "c_dev")}
    seen = {}
    for rep in range(args.warmup + args.reps):
        keep = rep >= args.warmup
        for v in variants:
            to_episode_end()
            if v == "a":
                t0 = time.perf_counter()
                r, l, ids = eng.finished_episodes()
                dt = {"a": time.perf_counter() - t0}
                seen[v] = len(r)
            elif v == "b":
                t0 = time.perf_counter()
                e0.record()
                fin = eng.finished_episodes_dev()
                st = eng.episode_stats_dev(fin)
                e1.record()
                torch.cuda.current_stream().synchronize()
                dt = {"b_wall": time.perf_counter() - t0, "b_dev": e0.elapsed_time(e1) * 1e-3}
                seen[v] = fin.count()
            elif v == "c_host":
                t0 = time.perf_counter()
                r, l, ids = eng.finished_episodes()
                ra, la = ptg_dist.all_gather_finished(r, l, device=dev)
                dt = {"c_host": time.perf_counter() - t0}
                seen[v] = len(ra)
            else:
                t0 = time.perf_counter()
                fin = eng.finished_episodes_dev()
                ra, la, ea = ptg_dist.all_gather_finished_dev(fin)
                torch.cuda.current_stream().synchronize()
                dt = {"c_dev": time.perf_counter() - t0}
                seen[v] = int(ra.numel())
            if keep:
                for k, x in dt.items():
                    times[k].append(x * 1e6)
    assert all(c == n for c in seen.values()), seen          # every variant handed out one episode per env
    print(f"# tools/fin_query.py: {n} envs, every env finishing on one step; {args.reps} repetitions after {args.warmup} warm-up, variants alternating")
    print(f"# block per rank: {ptg_dist.finished_block_nbytes(n)} bytes; torch {torch.__version__}; {torch.cuda.get_device_name(0)}")
    print(f"{'variant':8s} {'median_us':>10s} {'min_us':>10s} {'max_us':>10s}  n")
    for k in ("a", "b_dev", "b_wall", "c_host", "c_dev"):
        x = times[k]
        if x:
            print(f"{k:8s} {statistics.median(x):10.1f} {min(x):10.1f} {max(x):10.1f}  {len(x)}")
    st = st.cpu().numpy()
    print(f"# statistic of the last drained list: count {st[0]:.0f}, mean return {st[1] / st[0]:.6f}, mean length {st[3] / st[0]:.1f}, "
          f"min {st[4]:.6f}, max {st[5]:.6f}")
    eng.close()
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
