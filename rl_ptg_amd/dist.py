"""Sharding of the env batch over the GPUs of one node.

Env instances are independent: GPU g of G owns the contiguous global env range [g*n, (g+1)*n) with its own
copy of the (~8 MB) tables and price series, and NO per-step communication.  The reference's only cross-env
coupling, the module-global `ep_index` (env/ptg_gym_env.py:9,487-493), has a closed form when the envs of a
vector step terminate together: env with GLOBAL index e takes eps_ind[N_total + e + m*N_total] at its m-th reset
(`episode_plan`).  The one collective is an all-gather of the finished-episode (return, length) lists for the
episodic-return statistic (SB3's rollout/ep_rew_mean) -- RCCL over xGMI on GPUs (backend "nccl"), gloo in CPU tests.
Two routes: `all_gather_finished` takes the host lists of HipEngine.finished_episodes(); `all_gather_finished_dev` /
`all_reduce_episode_stats` take the device block of HipEngine.finished_episodes_dev() and its statistic as they are.
"""
import numpy as np


def shard_range(n_total, world_size, rank):
    """Contiguous global env range of `rank`; n_total must divide evenly (weak scaling uses n_total = n * world_size)."""
    if n_total % world_size != 0:
        raise ValueError(f"n_total={n_total} is not divisible by world_size={world_size}")
    n = n_total // world_size
    return rank * n, (rank + 1) * n


def episode_plan(n_total, world_size, rank):
    """(first_ptr, stride) for ptg_set_episode_plan on this rank's shard."""
    lo, _ = shard_range(n_total, world_size, rank)
    return n_total + lo, n_total


def mixed_scenario_assignment(n_total, world_size, rank, n_sets):
    """Per-env market set for a mixed-scenario batch: global env e gets set e % n_sets."""
    lo, hi = shard_range(n_total, world_size, rank)
    return (np.arange(lo, hi) % n_sets).astype(np.uint8)


INLINE = 15          # finished episodes per rank that travel with the count in the first (usually only) collective

_PINNED = {}         # (numel, dtype) -> pinned host staging tensor (device collectives only)


def _pinned(numel, dtype, tag):
    import torch
    key = (numel, dtype, tag)
    t = _PINNED.get(key)
    if t is None:
        t = _PINNED[key] = torch.empty(numel, dtype=dtype).pin_memory()
    return t


def _gather_rows(x, dev, group, world):
    """x: CPU tensor [m, c], the same shape on every rank -> NumPy [world, m, c]: one collective.  On a GPU device the rows go
    through pinned staging buffers with asynchronous copies and ONE stream synchronisation (no pageable copies)."""
    import torch
    import torch.distributed as dist
    flat = x.reshape(-1)
    if dev.type == "cuda":
        src_h = _pinned(flat.numel(), flat.dtype, "src")
        dst_h = _pinned(flat.numel() * world, flat.dtype, "dst")
        src_h.copy_(flat)
        src = src_h.to(dev, non_blocking=True)
        out = torch.empty(flat.numel() * world, dtype=flat.dtype, device=dev)
        dist.all_gather_into_tensor(out, src, group=group)
        dst_h.copy_(out, non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()
        return dst_h.numpy().reshape((world,) + tuple(x.shape)).copy()
    out = torch.empty((world,) + tuple(x.shape), dtype=x.dtype)
    try:
        dist.all_gather_into_tensor(out.view(-1), flat.contiguous(), group=group)
    except (RuntimeError, NotImplementedError, AttributeError):       # backend without the flat form
        parts = [torch.empty_like(x) for _ in range(world)]
        dist.all_gather(parts, x.contiguous(), group=group)
        out = torch.stack(parts)
    return out.numpy()


def all_gather_finished(returns, lengths, device=None, group=None):
    """All-gather variable-length finished-episode lists over the process group.

    Returns (returns_all, lengths_all) ordered by rank.  ONE collective in the common cases: every rank sends [count, then its
    first INLINE (return, length) pairs] as 1 + 2 * INLINE float64; only when some rank finished more than INLINE episodes a second
    collective carries the remainders (padded to the longest).  With no initialised process group this is the identity."""
    import torch
    import torch.distributed as dist
    returns = np.asarray(returns, dtype=np.float64)
    lengths = np.asarray(lengths, dtype=np.int64)
    if not (dist.is_available() and dist.is_initialized()):
        return returns, lengths
    world = dist.get_world_size(group)
    dev = torch.device("cpu") if device is None else torch.device(device)
    c = len(returns)
    head = np.zeros((1, 1 + 2 * INLINE))
    head[0, 0] = c
    k = min(c, INLINE)
    head[0, 1:1 + 2 * k:2] = returns[:k]
    head[0, 2:2 + 2 * k:2] = lengths[:k]                    # episode lengths are far below 2**53: exact as float64
    heads = _gather_rows(torch.from_numpy(head), dev, group, world)[:, 0, :]
    counts = heads[:, 0].astype(np.int64)
    m = int(counts.max()) - INLINE
    rest = None
    if m > 0:                                 # rare: a rank with more than INLINE finished episodes since the last call
        payload = np.zeros((m, 2))
        if c > INLINE:
            payload[:c - INLINE, 0] = returns[INLINE:]
            payload[:c - INLINE, 1] = lengths[INLINE:]
        rest = _gather_rows(torch.from_numpy(payload), dev, group, world)
    r_all, l_all = [], []
    for rk in range(world):
        ck = int(counts[rk])
        kk = min(ck, INLINE)
        r_all.append(heads[rk, 1:1 + 2 * kk:2])
        l_all.append(heads[rk, 2:2 + 2 * kk:2].astype(np.int64))
        if ck > INLINE:
            r_all.append(rest[rk, :ck - INLINE, 0])
            l_all.append(rest[rk, :ck - INLINE, 1].astype(np.int64))
    return np.concatenate(r_all), np.concatenate(l_all)


def episode_boundary_in_window(steps_to_episode_end, n_steps, device=None, group=None):
    """Does an episode end within the next `n_steps` vector steps on ANY rank?  `steps_to_episode_end` is this rank's
    HipEngine.steps_to_episode_end() (0 = unknown to the host: a de-synchronised batch, where an episode may end on any step).  All
    ranks get the same answer (one all-reduce of a flag when a process group is up), so the finished-episode all-gather behind it is
    entered by everybody or by nobody.  SURVEY.md 8(e): the collective belongs to episode boundaries, not to the step path."""
    mine = steps_to_episode_end == 0 or steps_to_episode_end <= n_steps
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return bool(mine)
    import torch
    flag = torch.tensor([1.0 if mine else 0.0], dtype=torch.float64, device=torch.device("cpu") if device is None else torch.device(device))
    dist.all_reduce(flag, op=dist.ReduceOp.MAX, group=group)
    return bool(flag.item() > 0)


def merge_moments(parts):
    """Chan merge of per-shard moments: parts [world, T, 3] of (count, mean, M2) -> [T, 3], shards taken in rank order
    (every rank computes the same floating-point result).  NumPy arrays or torch tensors."""
    is_torch = hasattr(parts[0], "clone")
    first = parts[0].clone() if is_torch else np.array(parts[0], dtype=np.float64)
    c, m, M = first[..., 0], first[..., 1], first[..., 2]
    for p in parts[1:]:
        cb, mb, Mb = p[..., 0], p[..., 1], p[..., 2]
        tot = c + cb
        safe = tot + (tot == 0)                      # a step with no envs on either side stays (0, 0, 0)
        delta = mb - m
        m = m + delta * cb / safe
        M = M + Mb + delta * delta * c * cb / safe
        c = tot
    if is_torch:
        import torch
        return torch.stack([c, m, M], dim=-1)
    return np.stack([c, m, M], axis=-1)


def all_merge_moments(moments, group=None):
    """[T, 3] per-step (count, mean, M2) of this rank's envs -> the moments over all ranks' envs (identity without a process
    group): one all-gather, then merge_moments."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return moments
    import torch
    world = dist.get_world_size(group)
    src = moments.contiguous()
    if src.is_cuda and dist.get_backend(group) != "nccl":      # CPU-side backends (gloo rehearsals): collective on a host copy
        src = src.cpu()
    parts = [torch.empty_like(src) for _ in range(world)]
    dist.all_gather(parts, src, group=group)
    return merge_moments(torch.stack(parts)).to(moments.device).contiguous()


# ---- the device route: a fixed-size block per rank, one collective ("fixed-size N/G returns + lengths + a count") ----
FIN_HEAD = 16        # bytes in front of the arrays: counts uint32[2] = (entries in the list, entries dropped), padded to 16


def finished_block_nbytes(cap):
    """[counts u32 x 2 | pad to 16 | returns f64 x cap | lengths i32 x cap | env_ids i32 x cap]"""
    return FIN_HEAD + 16 * int(cap)


class FinishedBlock:
    """A finished-episode list as ONE contiguous uint8 tensor (`block`) and typed views of it: `counts` int32[2] (the library writes
    them as uint32; a list never holds 2**31 entries), `returns` float64[cap], `lengths` int32[cap], `env_ids` int32[cap] (global env
    indices).  Only the first counts[0] entries of the arrays mean anything.  The block is what travels in the collective."""

    def __init__(self, block, cap):
        import torch
        cap = int(cap)
        if block.dtype != torch.uint8 or block.dim() != 1 or block.numel() != finished_block_nbytes(cap) or not block.is_contiguous():
            raise ValueError(f"a finished-episode block of cap {cap} is a contiguous uint8 tensor of {finished_block_nbytes(cap)} bytes")
        self.block, self.cap = block, cap
        self.counts = block[0:8].view(torch.int32)
        self.returns = block[FIN_HEAD:FIN_HEAD + 8 * cap].view(torch.float64)
        self.lengths = block[FIN_HEAD + 8 * cap:FIN_HEAD + 12 * cap].view(torch.int32)
        self.env_ids = block[FIN_HEAD + 12 * cap:FIN_HEAD + 16 * cap].view(torch.int32)

    @classmethod
    def empty(cls, cap, device):
        """an empty list (all bytes zero) on `device`"""
        import torch
        return cls(torch.zeros(finished_block_nbytes(cap), dtype=torch.uint8, device=device), cap)

    def count(self):
        """entries in the list, on the host (synchronises a device block)"""
        return int(self.counts[0].item())

    def lists(self):
        """(returns, lengths, env_ids) trimmed to the count: views of the block (synchronises a device block for the count)"""
        c = min(self.count(), self.cap)
        return self.returns[:c], self.lengths[:c], self.env_ids[:c]


def pack_finished_block(returns, lengths, env_ids, cap, device=None, dropped=0):
    """The block HipEngine.finished_episodes_dev() fills, built from host lists (at most `cap` entries) -- for rehearsing the collective
    without a GPU, or for handing host-collected episodes to the device route."""
    import torch
    cap = int(cap)
    r = np.asarray(returns, dtype=np.float64).reshape(-1)
    l = np.asarray(lengths, dtype=np.int32).reshape(-1)
    e = np.asarray(env_ids, dtype=np.int32).reshape(-1)
    if not (len(r) == len(l) == len(e)) or len(r) > cap:
        raise ValueError(f"lists of {len(r)}, {len(l)}, {len(e)} entries do not make a block of cap {cap}")
    c = len(r)
    raw = np.zeros(finished_block_nbytes(cap), np.uint8)
    raw[0:8].view(np.uint32)[:] = (c, int(dropped))
    raw[FIN_HEAD:FIN_HEAD + 8 * cap].view(np.float64)[:c] = r
    raw[FIN_HEAD + 8 * cap:FIN_HEAD + 12 * cap].view(np.int32)[:c] = l
    raw[FIN_HEAD + 12 * cap:FIN_HEAD + 16 * cap].view(np.int32)[:c] = e
    block = torch.from_numpy(raw)
    if device is not None and torch.device(device).type != "cpu":
        block = block.to(device)
    return FinishedBlock(block, cap)


def _gather_flat(src, group):
    """src: contiguous 1-D tensor, the same size on every rank -> [world, numel] on src's device: ONE all_gather_into_tensor.  Under
    "nccl" the tensor goes in as it is; under a CPU backend (gloo rehearsals) a device tensor goes through a host copy, as in
    all_merge_moments."""
    import torch
    import torch.distributed as dist
    world = dist.get_world_size(group)
    x = src
    if x.is_cuda and dist.get_backend(group) != "nccl":
        x = x.cpu()
    out = torch.empty(world * x.numel(), dtype=x.dtype, device=x.device)
    dist.all_gather_into_tensor(out, x, group=group)
    return out.view(world, x.numel()).to(src.device)


def all_gather_finished_dev(fin, group=None):
    """All-gather the ranks' finished-episode blocks (FinishedBlock, the same cap on every rank): ONE collective of
    16 + 16 * cap bytes per rank whatever the counts are -- a synchronised batch whose envs all finish on one step included.
    Returns (returns_all, lengths_all, env_ids_all) in rank order, each rank's part trimmed to its count, as tensors on the block's
    device.  The counts come to the host (one small copy) to trim; the lists stay where the block is.  With no initialised process
    group this is the identity."""
    import torch
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return fin.lists()
    cap = fin.cap
    allb = _gather_flat(fin.block, group)                              # [world, nbytes]
    world = allb.shape[0]
    counts = allb[:, 0:4].contiguous().view(torch.int32).reshape(world).cpu().tolist()
    ret = allb[:, FIN_HEAD:FIN_HEAD + 8 * cap].contiguous().view(torch.float64)              # [world, cap]
    ln = allb[:, FIN_HEAD + 8 * cap:FIN_HEAD + 12 * cap].contiguous().view(torch.int32)
    ids = allb[:, FIN_HEAD + 12 * cap:FIN_HEAD + 16 * cap].contiguous().view(torch.int32)
    keep = [min(max(int(c), 0), cap) for c in counts]
    if all(c == cap for c in keep):                                     # every rank full: the gathered arrays are the lists
        return ret.reshape(-1), ln.reshape(-1), ids.reshape(-1)
    return (torch.cat([ret[k, :c] for k, c in enumerate(keep)]), torch.cat([ln[k, :c] for k, c in enumerate(keep)]),
            torch.cat([ids[k, :c] for k, c in enumerate(keep)]))


def merge_episode_stats(parts):
    """[world, 6] of {count, sum r, sum r^2, sum len, min r, max r} (a CPU tensor) -> [6]: the sums added in rank order, min / max
    folded in rank order -- every rank that holds the same parts computes the same bits."""
    acc = parts[0].clone()
    for p in parts[1:]:
        acc[0:4] = acc[0:4] + p[0:4]
        if p[4] < acc[4]:
            acc[4] = p[4]
        if p[5] > acc[5]:
            acc[5] = p[5]
    return acc


def all_reduce_episode_stats(stats, group=None):
    """The survey's other form of the collective: HipEngine.episode_stats_dev()'s float64[6] of this rank's list -> the statistic
    over all ranks' lists.  ONE gather of the 6 values per rank and a merge in rank order (merge_episode_stats), rather than an
    all-reduce(SUM) plus two for min / max: a single collective, and identical bits on every rank by construction instead of by the
    backend's reduction order.  The 6 x world numbers are folded on the host.  Identity without a process group."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return stats
    parts = _gather_flat(stats.contiguous().reshape(-1), group)
    return merge_episode_stats(parts.cpu()).to(stats.device)
