"""The device-side way out of the finished-episode ring (include/ptg_env.h: ptg_finished_episodes_dev, ptg_episode_stats_dev): a
stream-ordered drain into the caller's device arrays and Monitor's statistic of them (info["episode"] of SB3's Monitor, as the reference
wraps its envs in src/rl_utils.py:448-453), next to the host query ptg_finished_episodes.  Twin handles on the same
noise streams: one leaves through the host query, the other through the drain -- the same ring, so the same doubles."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OFFSET = 1000003                     # global index of env 0 (ptg_set_global_env_offset): the drain adds it, the ring holds local indices
CANARY_I = -1163005939               # 0xBAADF00D
CANARY_F = -1.2345678901234567e300
EPS = 2.0 ** -52                     # a float64 sum of n terms is within n * EPS * sum|x| of the exact one, in any order


def _pair(n, k=2, offset=OFFSET, **kw):
    """k handles on the 96-step episodes of tests/test_graph_replay.py (eps_len_d=4, sim_step=3600: the 91st call terminates)"""
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    kw.setdefault("sim_step", 3600)
    spec, _ = synthetic_spec(scenario=2, operation="OP2", eps_len_d=4, **kw)
    engs = []
    for _ in range(k):
        e = HipEngine(spec.consts, spec.tables, spec.markets, n, device=0, out_dtype="float32", obs_layout="row")
        e.set_episode_plan(spec.eps_ind, n, n)
        e.set_global_env_offset(offset)                   # keys the noise streams too: the same on every twin
        e.set_noise_rng(seed=77)
        engs.append(e)
    return [spec] + engs


def _actions(steps, n, seed):
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randint(0, 5, (steps, n), dtype=torch.int32, device="cuda", generator=g)


class _Stepper:
    """fused rollouts in chunks of T steps into buffers that are reused (the episode's terminating step runs on the generic kernel)"""

    def __init__(self, eng, T=13):
        import torch
        self.eng, self.T = eng, T
        self.obs = eng.alloc_obs(T)
        self.rew = torch.empty((T, eng.n), dtype=eng.out_dtype, device="cuda")
        self.done = torch.empty((T, eng.n), dtype=torch.uint8, device="cuda")

    def run(self, acts):
        for s in range(0, acts.shape[0], self.T):
            c = acts[s:s + self.T]
            t = c.shape[0]
            self.eng.rollout(c, self.obs[:t], self.rew[:t], self.done[:t])


class _Guarded:
    """The output arrays of a drain, each with a canary word in front of it and behind its `cap` entries, filled with canaries."""

    def __init__(self, cap):
        import torch
        self.cap = cap
        self.ret = torch.full((cap + 2,), CANARY_F, dtype=torch.float64, device="cuda")
        self.len = torch.full((cap + 2,), CANARY_I, dtype=torch.int32, device="cuda")
        self.env = torch.full((cap + 2,), CANARY_I, dtype=torch.int32, device="cuda")
        self.cnt = torch.full((4,), CANARY_I, dtype=torch.int32, device="cuda")

    def zero_counts(self):
        self.cnt[1:3] = 0

    def drain(self, eng, append=False, use=(True, True, True)):
        return eng._L.ptg_finished_episodes_dev(
            eng._h, C.c_void_p(self.ret.data_ptr() + 8) if use[0] else None, C.c_void_p(self.len.data_ptr() + 4) if use[1] else None,
            C.c_void_p(self.env.data_ptr() + 4) if use[2] else None, self.cap, C.c_void_p(self.cnt.data_ptr() + 4), 1 if append else 0,
            eng._stream())

    def stats(self, eng, stats, accumulate=False):
        return eng._L.ptg_episode_stats_dev(eng._h, C.c_void_p(self.ret.data_ptr() + 8), C.c_void_p(self.len.data_ptr() + 4),
                                            C.c_void_p(self.cnt.data_ptr() + 4), C.c_void_p(stats.data_ptr()), 1 if accumulate else 0,
                                            eng._stream())

    def read(self):
        """(returns, lengths, env ids, counts) on the host after checking that nothing outside [0, count) of any array was written"""
        import torch
        torch.cuda.synchronize()
        cnt = self.cnt.cpu().numpy()
        assert cnt[0] == CANARY_I and cnt[3] == CANARY_I, "canary beside the counts"
        c, dropped = int(cnt[1]), int(cnt[2])
        assert 0 <= c <= self.cap
        r, l, e = self.ret.cpu().numpy(), self.len.cpu().numpy(), self.env.cpu().numpy()
        can = np.float64(CANARY_F).view(np.int64)
        assert r[0].view(np.int64) == can and np.all(r[1 + c:].view(np.int64) == can), "returns: written outside the list"
        assert l[0] == CANARY_I and np.all(l[1 + c:] == CANARY_I), "lengths: written outside the list"
        assert e[0] == CANARY_I and np.all(e[1 + c:] == CANARY_I), "env ids: written outside the list"
        return r[1:1 + c].copy(), l[1:1 + c].copy(), e[1:1 + c].copy(), (c, dropped)


def _sorted(r, l, e):
    o = np.lexsort((r, l, e))                                 # by env id, then length, then return
    return r[o], l[o], e[o]


def _same_lists(got, exp, what=""):
    (r1, l1, e1), (r2, l2, e2) = _sorted(*got), _sorted(*exp)
    assert len(r1) == len(r2), (what, len(r1), len(r2))
    assert np.array_equal(e1, e2) and np.array_equal(l1, l2), what
    assert np.array_equal(r1.view(np.int64), r2.view(np.int64)), what + ": returns are not bit-equal"


def _np_stats(r, l):
    return np.array([len(r), np.sum(r), np.sum(r * r), np.sum(l.astype(np.float64)), np.min(r) if len(r) else np.inf,
                     np.max(r) if len(r) else -np.inf])


def _check_stats(got, r, l, what=""):
    exp = _np_stats(r, l)
    n = len(r)
    print(f"{what} stats got {got.tolist()} numpy {exp.tolist()}")
    assert got[0] == exp[0] and got[3] == exp[3] and got[4] == exp[4] and got[5] == exp[5], what
    assert abs(got[1] - exp[1]) <= n * EPS * np.sum(np.abs(r)), what
    assert abs(got[2] - exp[2]) <= n * EPS * np.sum(r * r), what


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000, 65536])
def test_drain_equals_host_query(n):
    """Two episode ends, then handle A's host query against handle B's drain: the same entries, bit for bit, with global env ids and
    nothing written outside the list; then a third episode end drained with a cap smaller than the list; then an empty ring.  The
    statistic of every drained list against NumPy, twice for the same bits."""
    import torch
    spec, A, B = _pair(n)
    A.reset(); B.reset()
    to_end = A.steps_to_episode_end()
    assert to_end == spec.consts["eps_sim_steps"] - 5 == 91
    acts = _actions(3 * to_end, n, seed=n)
    sa, sb = _Stepper(A), _Stepper(B)
    sa.run(acts[:2 * to_end]); sb.run(acts[:2 * to_end])
    ra, la, ea = A.finished_episodes()
    assert len(ra) == 2 * n and set(la.tolist()) == {to_end}
    g = _Guarded(2 * n)
    assert g.drain(B) == 0
    stats = torch.zeros((2, 6), dtype=torch.float64, device="cuda")
    assert g.stats(B, stats[0]) == 0 and g.stats(B, stats[1]) == 0
    rb, lb, eb, (c, dropped) = g.read()
    assert c == len(ra) and dropped == 0
    _same_lists((rb, lb, eb - OFFSET), (ra, la, ea), f"n={n}")
    assert eb.min() == OFFSET and eb.max() == OFFSET + n - 1
    st = stats.cpu().numpy()
    _check_stats(st[0], rb, lb, f"n={n}")
    assert st[0].tobytes() == st[1].tobytes()                                # the same list, the same bits
    assert B.finished_dropped() == 0                                         # the host counter counts host queries only
    # third episode end, cap smaller than the list: the drain keeps what fits, counts the rest as dropped, and empties the ring
    sa.run(acts[2 * to_end:]); sb.run(acts[2 * to_end:])
    ra, la, ea = A.finished_episodes()
    assert len(ra) == n
    small = max(1, n // 3)
    g2 = _Guarded(small)
    assert g2.drain(B) == 0
    rb, lb, eb, (c, dropped) = g2.read()
    assert c == small and dropped == n - small
    assert len(set(eb.tolist())) == small                                    # a subset of the host list, entry for entry
    pos = {int(e): i for i, e in enumerate(ea)}
    idx = np.array([pos[int(e) - OFFSET] for e in eb])
    assert np.array_equal(rb.view(np.int64), ra[idx].view(np.int64)) and np.array_equal(lb, la[idx])
    g3 = _Guarded(small)
    assert g3.drain(B) == 0 and g3.stats(B, stats[0]) == 0
    assert g3.read()[3] == (0, 0)                                            # the ring was emptied, dropped entries included
    assert stats[0].cpu().tolist() == [0.0, 0.0, 0.0, 0.0, np.inf, -np.inf]  # statistic of an empty list
    rh, lh, eh = B.finished_episodes()                                       # the host query after a drain: synchronises, finds nothing
    assert len(rh) == 0
    A.close(); B.close()


def test_drained_returns_against_the_oracle():
    """The mixed-scenario batch of tests/test_mixed_scenarios.py (three market sets, state-change penalty on, episode plan, float64)
    beside its three CPU oracles: the episode returns that leave through the drain are the oracle's sums of rewards within the
    project's bound for them, 1e-9 * sum|r|; lengths and env ids exact."""
    import torch
    import test_mixed_scenarios as TM
    specs = TM._specs_for(0.3)
    eps_ind = specs[0].eps_ind
    spec, eng, tape = TM._engine(specs, "float64", "row", "tape", seed=41)
    eng.set_episode_plan(eps_ind, TM.N, TM.N)
    ora = TM._Oracles(specs, tape, eps_ind)
    eng.reset(); ora.reset()
    acts = TM._sticky(np.random.default_rng(17), TM.K, TM.N)
    ret, abs_ret, length, exp = np.zeros(TM.N), np.zeros(TM.N), np.zeros(TM.N, np.int64), []
    for t in range(TM.K):
        _, r_ref, d_ref = ora.step(acts[t])
        ret += r_ref; abs_ret += np.abs(r_ref); length += 1
        for e in np.nonzero(d_ref)[0]:
            exp.append((int(e), int(length[e]), ret[e], abs_ret[e]))
        d = d_ref.astype(bool)
        ret[d], abs_ret[d], length[d] = 0.0, 0.0, 0
    assert len(exp) == 2 * TM.N
    from rl_ptg_amd.dist import FinishedBlock
    fin = FinishedBlock.empty(2 * TM.N, eng.device)
    for t0 in range(0, TM.K, 150):                                           # fused chunks, the list appended to behind each
        eng.rollout(acts[t0:t0 + 150])
        eng.finished_episodes_dev(block=fin, append=True)
    eng.sync()
    assert fin.counts.tolist() == [2 * TM.N, 0]
    r, l, ids = (x.cpu().numpy() for x in fin.lists())
    got = sorted(zip(ids.tolist(), l.tolist(), r.tolist()))
    worst = 0.0
    for (e1, l1, r1), (e2, l2, r2, a2) in zip(got, sorted(exp)):
        assert e1 == e2 and l1 == l2, (e1, e2, l1, l2)
        worst = max(worst, abs(r1 - r2) / a2)
        assert abs(r1 - r2) <= 1e-9 * a2, (e1, l1, r1, r2)
    print(f"drained returns vs oracle: worst |dr| / sum|r| = {worst:.3e} (bound 1e-9)")
    eng.close(); ora.close()


def test_append_is_the_concatenation_of_fresh_drains():
    import torch
    n = 257
    spec, A, B = _pair(n)
    A.reset(); B.reset()
    to_end = A.steps_to_episode_end()
    acts = _actions(3 * to_end, n, seed=3)
    sa, sb = _Stepper(A), _Stepper(B)
    gb = _Guarded(3 * n)
    gb.zero_counts()
    fresh = []
    for q in range(3):
        sa.run(acts[q * to_end:(q + 1) * to_end]); sb.run(acts[q * to_end:(q + 1) * to_end])
        ga = _Guarded(n)
        assert ga.drain(A) == 0 and gb.drain(B, append=True) == 0
        r, l, e, cnt = ga.read()
        assert cnt == (n, 0)
        fresh.append((r, l, e))
        assert gb.read()[3] == ((q + 1) * n, 0)
    r, l, e, _ = gb.read()
    for q in range(3):                                                       # segment q of the appended list = the q-th fresh drain
        _same_lists((r[q * n:(q + 1) * n], l[q * n:(q + 1) * n], e[q * n:(q + 1) * n]), fresh[q], f"segment {q}")
    assert not np.array_equal(fresh[0][0], fresh[1][0])                      # three different episodes (the plan moves on)
    # a full list takes nothing more: one more episode end is counted as dropped, and the ring is emptied all the same
    extra = _actions(to_end, n, seed=4)
    sb.run(extra)
    assert gb.drain(B, append=True) == 0
    r2, l2, e2, cnt = gb.read()
    assert cnt == (3 * n, n) and np.array_equal(r2.view(np.int64), r.view(np.int64))
    g0 = _Guarded(n)
    assert g0.drain(B) == 0 and g0.read()[3] == (0, 0)
    A.close(); B.close()


def test_ring_overflow_keeps_the_newest_and_counts_the_rest():
    """The dropped-counter recipe of tests/test_bench_path.py: 8 envs, 139-step episodes, 130 episode ends between two drains = 1 040
    finished episodes into a ring of max(2 n, 1024) = 1 024: the drain hands out the newest 1 024, as the host query does on the twin,
    and counts 16 dropped; with a cap of 1 000 it hands out the oldest 1 000 of those and counts 40."""
    import torch
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    spec, _ = synthetic_spec(scenario=2, operation="OP2", eps_len_d=1, train_steps=200000)
    n = 8
    engs = []
    for _ in range(3):
        e = HipEngine(spec.consts, spec.tables, spec.markets, n, device=0, out_dtype="float32", obs_layout="row")
        e.set_episode_plan(spec.eps_ind, n, n)
        e.set_noise_rng(3)
        e.reset()
        engs.append(e)
    A, B, B2 = engs
    ep_len = int(spec.consts["eps_sim_steps"]) - 5
    assert A.steps_to_episode_end() == ep_len == 139
    acts = _actions(ep_len, n, seed=0)
    steppers = [_Stepper(e, T=ep_len) for e in engs]
    n_eps = 130
    for _ in range(n_eps):
        for s in steppers:
            s.run(acts)
    finished = n_eps * n                                                     # every env finishes on the last step of every pass
    ra, la, ea = A.finished_episodes()
    assert len(ra) == 1024 and A.finished_dropped() == finished - 1024
    g = _Guarded(1024)
    assert g.drain(B) == 0
    rb, lb, eb, (c, dropped) = g.read()
    assert c + dropped == finished and c == 1024
    _same_lists((rb, lb, eb), (ra, la, ea), "newest 1024")
    # ring order is oldest first, so the host list's first 1000 are what a cap of 1000 keeps (one wave per step: the order is fixed)
    g2 = _Guarded(1000)
    assert g2.drain(B2) == 0
    r2, l2, e2, (c, dropped) = g2.read()
    assert c == 1000 and c + dropped == finished
    assert np.array_equal(r2.view(np.int64), ra[:1000].view(np.int64)) and np.array_equal(e2, ea[:1000]) and np.array_equal(l2, la[:1000])
    assert B.finished_dropped() == 0 and B2.finished_dropped() == 0
    for e in engs:
        e.close()


def test_drain_does_not_synchronise_the_host():
    """A condition, not a timing: 2 000 fused steps at 65 536 envs are about 3 ms of device time by the project's own figure (1.5 us per
    fused step at that width), some hundred times what the host needs to enqueue them and the drain.  The stream is busy
    before the drain call (so the check cannot pass on an idle stream) and still busy when drain + statistic have returned."""
    import torch
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    n, T, calls = 65536, 250, 8
    spec, _ = synthetic_spec(scenario=2, operation="OP2", eps_len_d=32)          # 4 608-step episodes: no boundary inside the 2 000 steps
    eng = HipEngine(spec.consts, spec.tables, spec.markets, n, device=0, out_dtype="float32", obs_layout="row")
    eng.set_episode_plan(spec.eps_ind, n, n)
    eng.set_noise_rng(5)
    eng.reset()
    assert eng.steps_to_episode_end() > T * calls + T
    acts = _actions(T, n, seed=1)
    st = _Stepper(eng, T=T)
    st.run(acts)                                                             # warm: first-launch work is not part of the condition
    fin = eng.finished_episodes_dev()
    stats = eng.episode_stats_dev(fin)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    assert stream.query() is True
    for _ in range(calls):
        st.run(acts)
    busy_before = stream.query()
    fin = eng.finished_episodes_dev()
    stats = eng.episode_stats_dev(fin)
    busy_after = stream.query()
    assert busy_before is False, "the rollouts were over before the drain was called: the check would prove nothing"
    assert busy_after is False, "the stream was idle when the drain returned: the call waited for the device"
    eng.sync()
    assert fin.counts.tolist() == [0, 0] and stats.cpu().tolist() == [0.0, 0.0, 0.0, 0.0, np.inf, -np.inf]
    eng.close()


def test_drain_between_generic_steps_changes_nothing():
    """A de-synchronised batch runs on the generic kernel, the one that pushes into the ring: a drain enqueued between two such steps
    leaves the second step's outputs and the state exactly as on the twin without a drain, and its list is the twin's host query."""
    import torch
    n = 300
    spec, A, B = _pair(n)
    A.reset(); B.reset()
    to_end = A.steps_to_episode_end()
    acts = _actions(to_end + 3, n, seed=8)
    _Stepper(A).run(acts[:to_end - 1]); _Stepper(B).run(acts[:to_end - 1])
    mask = (np.arange(n) % 5 == 0).astype(np.uint8)                          # every 5th env starts over: no common step count any more
    A.reset(mask); B.reset(mask)
    assert A.steps_to_episode_end() == 0 and B.steps_to_episode_end() == 0
    g = _Guarded(n)
    outs = []
    for eng in (A, B):
        o1, r1, d1 = (x.clone() for x in eng.step(acts[to_end - 1]))          # the other 240 envs terminate here
        if eng is B:
            assert g.drain(B) == 0
        o2, r2, d2 = (x.clone() for x in eng.step(acts[to_end]))
        if eng is B:
            assert g.drain(B, append=True) == 0
        o3, r3, d3 = (x.clone() for x in eng.step(acts[to_end + 1]))
        outs.append((o1, r1, d1, o2, r2, d2, o3, r3, d3))
    torch.cuda.synchronize()
    assert int(outs[0][2].sum()) == n - int(mask.sum())
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    for f in ("meth_state", "i", "j", "k", "noise_count", "act_ep_d", "cum_rew", "ep_ptr", "n_state_changes"):
        assert np.array_equal(A.get_state(f), B.get_state(f)), f
    ra, la, ea = A.finished_episodes()
    rb, lb, eb, cnt = g.read()
    assert cnt == (n - int(mask.sum()), 0)
    _same_lists((rb, lb, eb - OFFSET), (ra, la, ea))
    A.close(); B.close()


def test_step_drain_and_statistic_captured_as_one_graph():
    """ptg_set_replay_proof, then ptg_step + drain (append) + statistic (accumulate) captured as ONE graph and replayed over two and a half
    episodes.  The twin steps eagerly and asks the host after every step.  The appended list is the twin's list.  The statistic
    accumulates what every replay saw: replay t merges the statistic of the whole list as it stands after step t (an appended list is
    not cleared), so the expected value is the sum over t of the statistic of the twin's list after step t."""
    import torch
    n = 300
    spec, A, B = _pair(n)
    B.set_replay_proof(True)
    to_end = spec.consts["eps_sim_steps"] - 5
    R = 2 * to_end + 40
    acts = _actions(R + 4, n, seed=9)
    A.reset(); B.reset()
    act_buf = torch.zeros(n, dtype=torch.int32, device="cuda")
    obs, rew, done = B.alloc_obs(1)[0], torch.zeros(n, dtype=B.out_dtype, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    g = _Guarded(3 * n)
    g.zero_counts()
    stats = torch.tensor([0.0, 0.0, 0.0, 0.0, float("inf"), float("-inf")], dtype=torch.float64, device="cuda")

    def body():
        B.step(act_buf, obs, rew, done, want_final=False)
        assert g.drain(B, append=True) == 0
        assert g.stats(B, stats, accumulate=True) == 0

    act_buf.copy_(acts[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            body()
    torch.cuda.current_stream().wait_stream(side)
    rs, ls, es = [], [], []
    exp = np.array([0.0, 0.0, 0.0, 0.0, np.inf, -np.inf])
    terms, abs_r, abs_r2 = 0, 0.0, 0.0
    for t in range(R):
        act_buf.copy_(acts[t])
        graph.replay()
        o_ref, r_ref, d_ref = A.step(acts[t], want_final=False)
        torch.cuda.synchronize()
        assert torch.equal(done, d_ref) and torch.equal(rew, r_ref) and torch.equal(obs, o_ref), f"replay {t}"
        r, l, e = A.finished_episodes()
        rs.append(r); ls.append(l); es.append(e)
        rl, ll = np.concatenate(rs), np.concatenate(ls)
        s = _np_stats(rl, ll)
        exp[:4] += s[:4]
        exp[4], exp[5] = min(exp[4], s[4]), max(exp[5], s[5])
        terms += len(rl); abs_r += np.sum(np.abs(rl)); abs_r2 += np.sum(rl * rl)
    B.note_replays(R - 1)
    assert A.steps_to_episode_end() == B.steps_to_episode_end()
    rb, lb, eb, cnt = g.read()
    assert cnt == (2 * n, 0)
    ra, la, ea = np.concatenate(rs), np.concatenate(ls), np.concatenate(es)
    for q in range(2):                                                       # in the order the episodes ended, as the twin saw them
        _same_lists((rb[q * n:(q + 1) * n], lb[q * n:(q + 1) * n], eb[q * n:(q + 1) * n] - OFFSET),
                    (ra[q * n:(q + 1) * n], la[q * n:(q + 1) * n], ea[q * n:(q + 1) * n]), f"episode end {q}")
    got = stats.cpu().numpy()
    print(f"captured statistic {got.tolist()} expected {exp.tolist()} over {terms} terms")
    assert got[0] == exp[0] == terms and got[3] == exp[3] and got[4] == exp[4] and got[5] == exp[5]
    assert abs(got[1] - exp[1]) <= terms * EPS * abs_r and abs(got[2] - exp[2]) <= terms * EPS * abs_r2
    assert len(B.finished_episodes()[0]) == 0                                # everything left through the graph's drains
    for t in range(R, R + 4):                                                # eager calls behind the replays: both handles in step
        xa = A.step(acts[t], want_final=False)
        xb = B.step(acts[t], want_final=False)
        torch.cuda.synchronize()
        assert all(torch.equal(p, q) for p, q in zip(xa, xb))
    A.close(); B.close()


def test_engine_block_layout_and_views():
    """HipEngine.finished_episodes_dev: one contiguous uint8 block [counts | pad | returns | lengths | env ids] of cap n_envs, allocated
    once and reused; episode_stats_dev on it; the lists equal the twin's host query."""
    import torch
    from rl_ptg_amd import dist as ptg_dist
    n = 65
    spec, A, B = _pair(n)
    A.reset(); B.reset()
    to_end = A.steps_to_episode_end()
    acts = _actions(to_end, n, seed=2)
    _Stepper(A).run(acts); _Stepper(B).run(acts)
    fin = B.finished_episodes_dev()
    stats = B.episode_stats_dev(fin)
    assert B.finished_episodes_dev() is fin and fin.cap == n                 # second drain: the same block, now an empty list
    assert fin.block.dtype == torch.uint8 and fin.block.numel() == ptg_dist.finished_block_nbytes(n) == 16 + 16 * n and fin.block.is_contiguous()
    base = fin.block.data_ptr()
    assert (fin.counts.data_ptr(), fin.returns.data_ptr(), fin.lengths.data_ptr(), fin.env_ids.data_ptr()) == \
        (base, base + 16, base + 16 + 8 * n, base + 16 + 12 * n)
    B.sync()
    assert fin.counts.tolist() == [0, 0]
    ra, la, ea = A.finished_episodes()
    rb, lb, eb = fin.returns.cpu().numpy(), fin.lengths.cpu().numpy(), fin.env_ids.cpu().numpy()      # the first drain's entries are still there
    _same_lists((rb, lb, eb - OFFSET), (ra, la, ea))
    _check_stats(stats.cpu().numpy(), rb, lb, "engine block")
    packed = ptg_dist.pack_finished_block(rb, lb, eb, n, device="cuda")      # the host-built block is the same bytes behind the counts
    assert torch.equal(packed.block[16:], fin.block[16:]) and packed.counts.tolist() == [n, 0]
    A.close(); B.close()


def test_bad_arguments_enqueue_nothing():
    import torch
    n = 64
    spec, A, B = _pair(n)
    A.close()
    B.reset()
    acts = _actions(B.steps_to_episode_end(), n, seed=6)
    _Stepper(B).run(acts)
    g = _Guarded(n)
    stats = torch.zeros(6, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()                                                            # the stream is idle from here on
    assert torch.cuda.current_stream().query() is True
    L, h, st = B._L, B._h, B._stream()
    ret, ln, env, cnt = (C.c_void_p(g.ret.data_ptr() + 8), C.c_void_p(g.len.data_ptr() + 4), C.c_void_p(g.env.data_ptr() + 4),
                         C.c_void_p(g.cnt.data_ptr() + 4))
    assert L.ptg_finished_episodes_dev(h, ret, ln, env, n, None, 0, st) == -1           # PTG_E_INVALID: null count_dev
    assert L.ptg_finished_episodes_dev(h, ret, ln, env, 0, cnt, 0, st) == -1            # cap = 0
    assert L.ptg_finished_episodes_dev(h, None, None, None, n, cnt, 0, st) == -1        # all three arrays null
    assert b"bad argument" in L.ptg_last_error(h)
    assert L.ptg_episode_stats_dev(h, None, ln, cnt, C.c_void_p(stats.data_ptr()), 0, st) == -1
    assert L.ptg_episode_stats_dev(h, ret, ln, None, C.c_void_p(stats.data_ptr()), 0, st) == -1
    assert L.ptg_episode_stats_dev(h, ret, ln, cnt, None, 0, st) == -1
    assert torch.cuda.current_stream().query() is True                                  # nothing was enqueued
    assert g.cnt.cpu().tolist() == [CANARY_I] * 4 and stats.cpu().tolist() == [0.0] * 6
    assert g.drain(B, use=(True, False, False)) == 0                                    # one array is enough; the ring was not touched
    torch.cuda.synchronize()
    assert g.cnt.cpu().tolist()[1:3] == [n, 0]
    assert np.all(g.len.cpu().numpy() == CANARY_I) and np.all(g.env.cpu().numpy() == CANARY_I)
    assert np.all(g.ret.cpu().numpy()[1:n + 1] != CANARY_F) and g.ret.cpu().numpy()[n + 1] == CANARY_F
    B.close()


RCCL_SCRIPT = r'''
import os, sys
sys.path.insert(0, os.environ["PTG_ROOT"])
import numpy as np, torch, torch.distributed as dist
from rl_ptg_amd import dist as ptg_dist
from rl_ptg_amd.engine import HipEngine
from rl_ptg_amd.prep import synthetic_spec
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
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
    spec, _ = synthetic_spec(scenario=2, operation="OP2", eps_len_d=4, sim_step=3600)
    n = 1000
    eng = HipEngine(spec.consts, spec.tables, spec.markets, n, device=0, out_dtype="float32", obs_layout="row")
    eng.set_episode_plan(spec.eps_ind, *ptg_dist.episode_plan(n, 1, 0))
    eng.set_global_env_offset(4096)
    eng.set_noise_rng(3)
    eng.reset()
    acts = np.random.default_rng(5).integers(0, 5, (eng.steps_to_episode_end(), n)).astype(np.int32)
    eng.rollout(acts)
    fin = eng.finished_episodes_dev()
    stats = eng.episode_stats_dev(fin)
    ra, la, ea = ptg_dist.all_gather_finished_dev(fin)
    assert calls["n"] == 1, calls
    assert ra.device.type == "cuda" and la.dtype == torch.int32 and ea.dtype == torch.int32 and ra.dtype == torch.float64
    assert fin.counts.tolist() == [n, 0] and ra.shape == (n,)
    assert torch.equal(ra, fin.returns) and torch.equal(la, fin.lengths) and torch.equal(ea, fin.env_ids)
    assert sorted(ea.tolist()) == list(range(4096, 4096 + n))
    st = ptg_dist.all_reduce_episode_stats(stats)
    assert calls["n"] == 2 and st.device.type == "cuda"
    assert st.cpu().numpy().tobytes() == stats.cpu().numpy().tobytes()
    fin = eng.finished_episodes_dev()                       # an empty list through the same collective
    ra, la, ea = ptg_dist.all_gather_finished_dev(fin)
    assert calls["n"] == 3 and ra.numel() == 0 and la.numel() == 0 and ea.numel() == 0
    eng.close()
    print("RCCL_DEV_OK")
finally:
    if dist.is_initialized():
        dist.destroy_process_group()
'''


def test_device_block_on_the_rccl_backend_one_rank():
    """One GPU, so one rank: a really drained block goes into RCCL as it is (device uint8), comes back unchanged, in one collective."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), PTG_ROOT=root, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, "-c", RCCL_SCRIPT], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "RCCL_DEV_OK" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
