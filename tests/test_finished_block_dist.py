"""The device route of the finished-episode collective, rehearsed on CPU with gloo (world size 2 and 8): every rank contributes ONE
fixed-size block (rl_ptg_amd.dist.FinishedBlock: counts, returns, lengths, global env ids) and one all_gather_into_tensor carries it
whatever the counts are -- ragged, a rank with nothing, and every rank full (the synchronised batch, whose envs all finish on one step:
the case that costs all_gather_finished two collectives).  all_reduce_episode_stats is the survey's other form: Monitor's statistic of
all ranks' lists from one gather of six numbers per rank, the same bits on every rank."""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from rl_ptg_amd import dist as ptg_dist


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _lists(rank, count, seed):
    """rank's finished episodes: returns of mixed sign and magnitude, lengths, global env ids of a 65 536-env shard"""
    rng = np.random.default_rng(seed * 1000 + rank)
    r = rng.normal(-40.0, 300.0, count)
    l = rng.integers(1, 5000, count).astype(np.int32)
    e = (rank * 65536 + rng.permutation(65536)[:count]).astype(np.int32)
    return r, l, e


def _stats_of(r, l):
    """what ptg_episode_stats_dev gives for a list (NumPy stands in for the kernel on the CPU)"""
    return torch.tensor([float(len(r)), float(np.sum(r)), float(np.sum(r * r)), float(np.sum(l.astype(np.float64))),
                         float(np.min(r)) if len(r) else float("inf"), float(np.max(r)) if len(r) else float("-inf")], dtype=torch.float64)


# (name, cap, count of `rank` in a world of `world`)
CASES = [("ragged", 64, lambda rank, world: rank + 2),
         ("one_empty", 64, lambda rank, world: 0 if rank == world - 1 else 5 + rank),
         ("all_empty", 16, lambda rank, world: 0),
         ("all_full", 300, lambda rank, world: 300)]
BIG = ("big_all_full", 65536, lambda rank, world: 65536)


def _cases(world):
    return CASES + ([BIG] if world == 8 else [])


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        calls = {"n": 0}
        real_flat, real_list = dist.all_gather_into_tensor, dist.all_gather

        def flat(*a, **k):
            calls["n"] += 1
            return real_flat(*a, **k)

        def lst(*a, **k):
            calls["n"] += 1
            return real_list(*a, **k)

        dist.all_gather_into_tensor, dist.all_gather = flat, lst
        out = {}
        for ci, (name, cap, count_of) in enumerate(_cases(world)):
            r, l, e = _lists(rank, count_of(rank, world), ci)
            fin = ptg_dist.pack_finished_block(r, l, e, cap)
            assert fin.block.numel() == 16 + 16 * cap and fin.count() == len(r)
            before = calls["n"]
            ra, la, ea = ptg_dist.all_gather_finished_dev(fin)
            n_gather = calls["n"] - before
            before = calls["n"]
            st = ptg_dist.all_reduce_episode_stats(_stats_of(r, l))
            n_stats = calls["n"] - before
            big = cap > 1000                                 # the big case travels back as digests, not as 8 x 524 288 numbers
            out[name] = dict(n_gather=n_gather, n_stats=n_stats, stats=st.numpy().tobytes(),
                             ret=ra.numpy().tobytes() if not big else None, len=la.numpy().tobytes() if not big else None,
                             ids=ea.numpy().tobytes() if not big else None,
                             dtypes=(str(ra.dtype), str(la.dtype), str(ea.dtype)), shapes=(tuple(ra.shape), tuple(la.shape), tuple(ea.shape)))
            if big:                                          # compared in the worker: every rank rebuilds every rank's list
                exp = [_lists(k, count_of(k, world), ci) for k in range(world)]
                out[name]["equal"] = (np.array_equal(ra.numpy(), np.concatenate([x[0] for x in exp])) and
                                      np.array_equal(la.numpy(), np.concatenate([x[1] for x in exp])) and
                                      np.array_equal(ea.numpy(), np.concatenate([x[2] for x in exp])))
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def _run(world):
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = sorted((q.get(timeout=300) for _ in range(world)), key=lambda x: x[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for ci, (name, cap, count_of) in enumerate(_cases(world)):
        exp = [_lists(k, count_of(k, world), ci) for k in range(world)]
        r_all = np.concatenate([x[0] for x in exp])
        l_all = np.concatenate([x[1] for x in exp])
        e_all = np.concatenate([x[2] for x in exp])
        n = len(r_all)
        for rank, res in out:
            c = res[name]
            assert c["n_gather"] == 1, (name, rank, c["n_gather"])          # ONE collective whatever the counts are
            assert c["n_stats"] == 1, (name, rank, c["n_stats"])
            assert c["dtypes"] == ("torch.float64", "torch.int32", "torch.int32")
            assert c["shapes"] == ((n,), (n,), (n,)), (name, rank, c["shapes"])
            if c["ret"] is None:
                assert c["equal"], (name, rank)
            else:                                                           # the concatenation in rank order, exactly
                assert c["ret"] == r_all.tobytes() and c["len"] == l_all.tobytes() and c["ids"] == e_all.tobytes(), (name, rank)
            st = np.frombuffer(c["stats"], np.float64)
            assert st[0] == n and st[3] == float(l_all.astype(np.int64).sum())
            if n:
                assert st[4] == r_all.min() and st[5] == r_all.max()
                # a float64 sum of n terms is within n * 2^-52 * sum|x| of the exact one, in any order
                eps = 2.0 ** -52
                assert abs(st[1] - np.sum(r_all)) <= n * eps * np.sum(np.abs(r_all)), (name, rank)
                assert abs(st[2] - np.sum(r_all * r_all)) <= n * eps * np.sum(r_all * r_all), (name, rank)
            else:
                assert st[1] == 0 and st[2] == 0 and st[4] == np.inf and st[5] == -np.inf
            assert c["stats"] == out[0][1][name]["stats"], (name, rank)     # bit-identical on every rank


def test_finished_block_world_size_2_gloo():
    _run(2)


def test_finished_block_world_size_8_gloo():
    _run(8)


def test_pack_finished_block_layout():
    r, l, e = np.array([1.5, -2.25, 3.0]), np.array([10, 20, 30]), np.array([70000, 5, 65536])
    fin = ptg_dist.pack_finished_block(r, l, e, cap=5, dropped=7)
    raw = fin.block.numpy()
    assert raw.dtype == np.uint8 and raw.shape == (16 + 16 * 5,) and ptg_dist.finished_block_nbytes(5) == 96
    assert raw[0:8].view(np.uint32).tolist() == [3, 7] and not raw[8:16].any()          # counts, then the pad to 16
    assert raw[16:56].view(np.float64).tolist() == [1.5, -2.25, 3.0, 0.0, 0.0]
    assert raw[56:76].view(np.int32).tolist() == [10, 20, 30, 0, 0]
    assert raw[76:96].view(np.int32).tolist() == [70000, 5, 65536, 0, 0]
    assert fin.counts.tolist() == [3, 7] and fin.cap == 5
    fin.returns[3] = 9.0                                                                # views of the one block, not copies
    assert raw[16:56].view(np.float64)[3] == 9.0
    for bad in (lambda: ptg_dist.pack_finished_block(r, l, e, cap=2), lambda: ptg_dist.pack_finished_block(r, l[:2], e, cap=5),
                lambda: ptg_dist.FinishedBlock(torch.zeros(95, dtype=torch.uint8), 5)):
        try:
            bad()
        except ValueError:
            continue
        raise AssertionError("a malformed block was accepted")


def test_no_process_group_is_the_identity():
    r, l, e = _lists(3, 9, 1)
    fin = ptg_dist.pack_finished_block(r, l, e, cap=32)
    ra, la, ea = ptg_dist.all_gather_finished_dev(fin)
    assert np.array_equal(ra.numpy(), r) and np.array_equal(la.numpy(), l) and np.array_equal(ea.numpy(), e)
    st = _stats_of(r, l)
    assert ptg_dist.all_reduce_episode_stats(st) is st
