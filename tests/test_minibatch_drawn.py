"""ptg_minibatch_drawn / ptg_minibatch_end_epoch, HipEngine.minibatch_drawn and DeviceRolloutBuffer.next_batch (include/ptg_env.h): a PPO /
A2C minibatch whose indices the gather computes itself from a device cursor {epoch, batch}, so that one captured gradient step replays
through every minibatch of every epoch.

Three exact comparisons, none with a tolerance: the indices against the Python-integer restatement of the header's permutation
(tests/minibatch_drawn_restatement.py, pinned by tests/test_minibatch_drawn_host.py), integer for integer; the union of an epoch's
indices against range(T * N); and observations and columns against HipEngine.minibatch at those indices, byte for byte through
integer views -- the gather is ptg_minibatch's own kernel behind another index source, and a copy has no rounding.  Payloads are
tests/test_minibatch.py's: random bits with NaN payloads, infinities, -0.0 and subnormals planted."""
import ctypes as C
import functools

import numpy as np
import pytest

import minibatch_drawn_restatement as md
import minibatch_restatement as mr
from test_minibatch import _bits, _engine, _equal_state, _fill_obs, _host_bits, _same

pytestmark = pytest.mark.gpu

SEED = 0x5EED0000F00D                                       # above 32 bits: both halves of the seed key the draw
# T, N, batch sizes, (layout, raw_modified, F), observation dtype, engine keywords, column element sizes
SHAPES = [
    (1, 1, [1], ("sb3_flat", "mod", 40), "float32", {}, [4]),
    (5, 3, [5], ("sb3_flat", "raw", 31), "float32", {}, [1, 2, 4, 8, 1, 2, 4, 8]),
    (7, 9, [1, 9, 21, 63], ("split", "mod", 16), "float64", {}, [8, 1]),
    (8, 8, [16, 64], ("feature", "mod", None), "float32", {"obs_pitch": 11}, []),
    (5, 13, [13, 65], ("feature", "mod", None), "float64", {"obs_pitch": 16}, [2]),
    (17, 3, [17], ("split", "mod", 16), "float32", {}, [4, 4]),                         # one row past a wave's 16
    (63, 65, [63], ("sb3_flat", "raw", 31), "float64", {}, [4]),
    (64, 64, [256], ("sb3_flat", "mod", 40), "float32", {}, [8, 4, 4, 4, 4]),           # four whole workgroups
    (17, 241, [241], ("row", "mod", 35), "float32", {}, [1]),
    (4263, 6, [203], ("sb3_flat", "mod", 40), "float32", {}, [8, 4, 4, 4, 4]),          # the reference's PPO: n_steps = 21 * 203, 6 envs
]


@functools.lru_cache(maxsize=None)
def _order(TN, seed, epoch):
    """the restated order of one epoch, computed once per (TN, seed, epoch) and never written to"""
    p = md.perm(TN, seed, epoch)
    p.setflags(write=False)
    return p


def _expected_batches(TN, B, seed, n):
    """the first n batches from cursor (0, 0) on: int64 [n, B]"""
    per = TN // B
    return np.stack([_order(TN, seed, k // per)[(k % per) * B:(k % per + 1) * B] for k in range(n)])


def _tdt(size):
    import torch
    return {1: torch.uint8, 2: torch.int16, 4: torch.float32, 8: torch.float64}[size]


@pytest.mark.parametrize("case", range(len(SHAPES)), ids=[f"{s[0]}x{s[1]}" for s in SHAPES])
def test_two_epochs_and_a_batch_of_the_third_are_exact(case):
    """row widths 40, 31 and 16 (split rows), feature-major with a pitch; float32 and float64; 0 to 8 columns of 1 to 8 bytes"""
    import torch
    T, N, Bs, (layout, rm, F), dtype, kw, col_sizes = SHAPES[case]
    eng = _engine(N, layout, rm, dtype, **kw)
    assert F in (None, eng.obs_dim) and eng.n == N and (not kw or eng.pitch == kw["obs_pitch"])
    F = eng.obs_dim
    size = 4 if dtype == "float32" else 8
    rng = np.random.default_rng([T, N, F, size])
    x = _bits((T, N, F), size, rng)
    obs = _fill_obs(eng, T, x)
    host_cols = [_bits((T, N), s, rng) for s in col_sizes]
    cols = [torch.from_numpy(h).cuda().view(_tdt(h.itemsize)) for h in host_cols]
    TN = T * N
    iv = torch.int32 if size == 4 else torch.int64
    for B in Bs:
        per = TN // B
        n = 2 * per + 1
        cur = eng.new_epoch_cursor()
        idx = torch.full((n, B), -1, dtype=torch.int64, device="cuda")
        od, om = torch.zeros((n, B, F), dtype=obs.dtype, device="cuda"), torch.zeros((n, B, F), dtype=obs.dtype, device="cuda")
        cd = [torch.zeros((n, B), dtype=c.dtype, device="cuda") for c in cols]
        cm = [torch.zeros((n, B), dtype=c.dtype, device="cuda") for c in cols]
        for k in range(n):
            got = eng.minibatch_drawn(cur, B, obs, cols, seed=SEED, obs_out=od[k], columns_out=[c[k] for c in cd], idx_out=idx[k])
            assert got[0].data_ptr() == od[k].data_ptr() and got[2].data_ptr() == idx[k].data_ptr()
            eng.minibatch(idx[k], obs, cols, obs_out=om[k], columns_out=[c[k] for c in cm])
        eng.sync()                                           # raises if a row was flagged
        what = f"T={T} N={N} B={B} F={F} {dtype} {layout}"
        got_idx = idx.cpu().numpy()
        np.testing.assert_array_equal(got_idx, _expected_batches(TN, B, SEED, n), err_msg=what)
        for e in range(2):
            np.testing.assert_array_equal(np.sort(got_idx[e * per:(e + 1) * per].reshape(-1)), np.arange(TN), err_msg=what)
        assert cur.tolist() == [2, 1] if per > 1 else cur.tolist() == [3, 0], (what, cur.tolist())
        assert torch.equal(od.view(iv), om.view(iv)), what
        for c, (a, b) in enumerate(zip(cd, cm)):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (what, c)
        # and the restatement of the gather itself, on the host
        _same(od[0], mr.gather(x, got_idx[0]), what)
        for c, h in enumerate(host_cols):
            _same(cd[c][n - 1], mr.gather(h, got_idx[n - 1]), what)
    eng.close()


def test_above_2_to_the_32_rows():
    """columns only, one uint8 column [65 537, 65 536] (4 GiB), one batch of 65 537 rows: positions, walks and values take the 64-bit
    path (33 bits: a = 16, b = 17).  Element (t, e) holds (131 t + 7 e) mod 251."""
    import torch
    T, N, B = 65537, 65536, 65537
    free = torch.cuda.mem_get_info()[0]
    if free < 6 * 2 ** 30:
        print(f"test_above_2_to_the_32_rows skipped: {free / 2 ** 30:.2f} GiB of device memory free, 6 GiB needed")
        pytest.skip(f"{free / 2 ** 30:.2f} GiB of device memory free, 6 GiB needed")
    eng = _engine(N, "sb3_flat", "mod", "float32")
    TN = T * N
    assert TN > 2 ** 32 and TN % B == 0
    col = torch.empty((T, N), dtype=torch.uint8, device="cuda")
    e7 = torch.arange(N, dtype=torch.int32, device="cuda")[None, :] * 7
    for a in range(0, T, 2048):
        b = min(a + 2048, T)
        col[a:b] = ((torch.arange(a, b, dtype=torch.int32, device="cuda")[:, None] * 131 + e7) % 251).to(torch.uint8)
    cur = eng.new_epoch_cursor()
    cur.copy_(torch.tensor([3, 65535]))                      # the epoch's last batch: positions up to T * N - 1
    out, idx = torch.zeros(B, dtype=torch.uint8, device="cuda"), torch.zeros(B, dtype=torch.int64, device="cuda")
    eng.minibatch_drawn(cur, B, None, [col], seed=SEED, columns_out=[out], idx_out=idx)
    eng.sync()
    assert cur.tolist() == [4, 0]
    keys = md.round_keys(SEED, 3)
    exp = np.array([md.perm_at(65535 * B + l, TN, keys) for l in range(B)], dtype=np.int64)
    got = idx.cpu().numpy()
    np.testing.assert_array_equal(got, exp)
    assert len(np.unique(got)) == B and 65535 * B == 2 ** 32 - 1
    t, e = exp % T, exp // T
    np.testing.assert_array_equal(out.cpu().numpy(), ((131 * t + 7 * e) % 251).astype(np.uint8))
    del col
    eng.close()
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------- the buffer's epoch cursor
def _filled_buffer(eng, T, seed, rng):
    """a DeviceRolloutBuffer whose window holds random bits; the int64 actions column holds each row's own flat index e * T + t, so a
    batch's actions ARE its indices"""
    import torch
    from rl_ptg_amd import DeviceRolloutBuffer
    N = eng.n
    buf = DeviceRolloutBuffer(eng, T, seed=seed)
    x = _bits((T, N, eng.obs_dim), 4, rng)
    eng.rows(buf.observations).view(torch.int32).copy_(torch.from_numpy(x).cuda())
    tag = (np.arange(N)[None, :] * T + np.arange(T)[:, None]).astype(np.int64)
    buf.actions.copy_(torch.from_numpy(tag).cuda())
    host = {"obs": x, "actions": tag}
    for name, t in (("values", buf.values), ("log_probs", buf.log_probs), ("advantages", buf.advantages), ("returns", buf.returns)):
        host[name] = _bits((T, N), 4, rng)
        t.view(torch.int32).copy_(torch.from_numpy(host[name]).cuda())
    return buf, host


def _check_batch(batch, host, idx, what=""):
    _same(batch.actions, idx.astype(np.int64), what + " indices")
    _same(batch.observations, mr.gather(host["obs"], idx), what + " observations")
    for name, got in (("values", batch.old_values), ("log_probs", batch.old_log_prob), ("advantages", batch.advantages), ("returns", batch.returns)):
        _same(got, mr.gather(host[name], idx), what + " " + name)


def test_next_batch_captured_alone_replays_through_an_epoch_boundary():
    """T x N = 8 x 6, B = 16: three batches an epoch.  One eager call (batch 0), the capture (which runs nothing: the cursor proves it),
    three replays -- batches 1 and 2 of epoch 0 and batch 0 of epoch 1, each the restatement's -- and the cursor reads (1, 1)"""
    import torch
    T, N, B = 8, 6, 16
    eng = _engine(N, "sb3_flat", "mod", "float32")
    buf, host = _filled_buffer(eng, T, SEED, np.random.default_rng(3))
    exp = _expected_batches(T * N, B, SEED, 4)
    out = buf.next_batch(B)
    eng.sync()
    _check_batch(out, host, exp[0], "eager")
    assert buf.epoch_cursor() == (0, 1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            again = buf.next_batch(B, out=out)
    torch.cuda.current_stream().wait_stream(side)
    assert all(a is b for a, b in zip(out, again)) and buf.epoch_cursor() == (0, 1)
    for k in (1, 2, 3):
        graph.replay()
        torch.cuda.synchronize()
        _check_batch(out, host, exp[k], f"replay {k}")
    assert buf.epoch_cursor() == (1, 1) and buf.cursor() == (0, 0)
    eng.sync()
    eng.close()


def test_end_epoch_set_epoch_cursor_get_and_begin():
    """end_epoch in the middle of an epoch: the next batch is batch 0 of the next epoch; at a fresh epoch it changes nothing.
    set_epoch_cursor restores what epoch_cursor read.  get(drawn=True) is one epoch of next_batch; begin() leaves the cursor alone."""
    import torch
    T, N, B = 8, 6, 16
    eng = _engine(N, "sb3_flat", "mod", "float32")
    buf, host = _filled_buffer(eng, T, 7, np.random.default_rng(4))
    TN = T * N
    buf.end_epoch()
    assert buf.epoch_cursor() == (0, 0)
    first = buf.next_batch(B)
    buf.end_epoch()
    assert buf.epoch_cursor() == (1, 0)
    buf.end_epoch()
    assert buf.epoch_cursor() == (1, 0)
    nxt = buf.next_batch(B)
    eng.sync()
    _check_batch(first, host, _order(TN, 7, 0)[:B], "epoch 0 batch 0")
    _check_batch(nxt, host, _order(TN, 7, 1)[:B], "epoch 1 batch 0")
    saved = buf.epoch_cursor()
    assert saved == (1, 1)
    b1 = buf.next_batch(B)
    buf.set_epoch_cursor(*saved)
    assert buf.epoch_cursor() == saved
    b1_again = buf.next_batch(B)
    eng.sync()
    _check_batch(b1, host, _order(TN, 7, 1)[B:2 * B], "epoch 1 batch 1")
    _check_batch(b1_again, host, _order(TN, 7, 1)[B:2 * B], "epoch 1 batch 1 after the restore")
    buf.set_epoch_cursor(5, 0)
    buf.begin(buf.last_obs)                                  # SB3's reset(): the next window draws under the next epoch numbers
    eng.sync()
    assert buf.epoch_cursor() == (5, 0) and buf.cursor() == (0, 0)
    buf.observations.view(torch.int32).copy_(torch.from_numpy(host["obs"]).cuda())       # begin() rewrote row 0
    batches = list(buf.get(B, drawn=True))
    whole = list(buf.get(drawn=True))                        # A2C: one batch of everything, epoch 6
    eng.sync()
    assert len(batches) == 3 and len(whole) == 1 and buf.epoch_cursor() == (7, 0)
    assert len({b.observations.data_ptr() for b in batches}) == 3           # fresh outputs per yield
    for j, b in enumerate(batches):
        _check_batch(b, host, _order(TN, 7, 5)[j * B:(j + 1) * B], f"get batch {j}")
    _check_batch(whole[0], host, _order(TN, 7, 6), "get(None)")
    # a cursor past its epoch is never walked: the rows stay, the next sync reports PTG_E_INDEX once, the next epoch starts
    from rl_ptg_amd import _lib
    from rl_ptg_amd.engine import PtgError
    buf.set_epoch_cursor(9, 3)
    keep = _host_bits(b1.observations).copy()
    buf.next_batch(B, out=b1)
    with pytest.raises(PtgError) as ei:
        eng.sync()
    assert ei.value.code == _lib.E_INDEX
    eng.sync()
    assert buf.epoch_cursor() == (10, 0)
    _same(b1.observations, keep)
    eng.close()


# ---------------------------------------------------------------------------------------------- a whole captured PPO gradient step
def test_a_captured_ppo_gradient_step_replayed_through_two_epochs():
    """next_batch -> TrainMLPGroup(policy 40 -> 32 -> 5, value 40 -> 32 -> 1) -> ppo_loss -> backward() -> DeviceOptimizer.step() on a real
    sb3_flat engine of 6 envs, T = 8, B = 16: one eager step (batch 0 of epoch 0; it loads the code objects and builds the optimiser's
    tables, which a capture cannot), the capture, then five replays for the other batches of two epochs.  The twin takes the same six
    steps eagerly over get(batch_size, perm=<the restated order of that epoch>).  Every parameter is bit-equal after every step and
    has moved from its initial value."""
    import torch
    from torch import nn
    from rl_ptg_amd import DeviceOptimizer, DeviceRolloutBuffer, TrainMLPGroup, ppo_loss
    from test_rollout_buffer import _engine as real_engine
    T, N, B, F, A = 8, 6, 16, 40, 5
    TN = T * N
    eng = real_engine(N, "sb3_flat")
    buf = DeviceRolloutBuffer(eng, T, seed=SEED)
    g = torch.Generator(device="cuda"); g.manual_seed(9)
    eng.reset()
    buf.begin()
    for t in range(T):
        act = torch.randint(0, A, (N,), dtype=torch.int64, device="cuda", generator=g)
        obs, rew, done = eng.step(act)
        buf.add(obs, rew, done, actions=act, values=0.1 * torch.randn(N, device="cuda", generator=g),
                log_probs=-1.6 + 0.1 * torch.randn(N, device="cuda", generator=g))
    buf.compute_returns_and_advantage(0.1 * torch.randn(N, device="cuda", generator=g), 0.99, 0.95)
    eng.sync()
    assert buf.cursor() == (T, 0)

    class Step:
        def __init__(self):
            torch.manual_seed(21)
            self.pi = nn.Sequential(nn.Linear(F, 32), nn.Tanh(), nn.Linear(32, A)).cuda()
            self.vf = nn.Sequential(nn.Linear(F, 32), nn.Tanh(), nn.Linear(32, 1)).cuda()
            self.grp = TrainMLPGroup(eng, [self.pi, self.vf], batch=B)
            self.params = self.grp.parameters()
            for p in self.params:
                p.grad = torch.zeros_like(p)
            self.opt = DeviceOptimizer(eng, self.params, kind="adam", lr=3e-3, eps=1e-5, max_grad_norm=0.5, zero_grad=True)
            self.ws = eng.policy_loss_workspace(B)
            self.samples = None

        def __call__(self, batch):
            logits, values = self.grp(batch.observations)
            loss, _ = ppo_loss(eng, logits, values, batch.actions, batch.old_log_prob, batch.advantages, batch.returns, clip_range=0.2,
                               ent_coef=0.01, workspace=self.ws)
            loss.backward()
            self.opt.step()

        def drawn(self):
            self.samples = buf.next_batch(B, out=self.samples)
            self(self.samples)

        def bits(self):
            return [_host_bits(p.detach()).copy() for p in self.params]

    cap, twin = Step(), Step()
    start = cap.bits()
    assert all(np.array_equal(a, b) for a, b in zip(start, twin.bits()))
    eager = [b for e in range(2) for b in buf.get(B, perm=torch.from_numpy(np.array(_order(TN, SEED, e))).cuda())]
    assert len(eager) == 6
    cap.drawn()                                              # the eager step
    twin(eager[0])
    torch.cuda.synchronize()
    assert buf.epoch_cursor() == (0, 1)
    assert all(np.array_equal(a, b) for a, b in zip(cap.bits(), twin.bits())), "the eager step"
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            cap.drawn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert buf.epoch_cursor() == (0, 1)                      # capturing ran nothing
    for k in range(1, 6):
        graph.replay()
        twin(eager[k])
        torch.cuda.synchronize()
        _same(cap.samples.actions, _host_bits(eager[k].actions), f"step {k}: the batch")
        for i, (a, b) in enumerate(zip(cap.bits(), twin.bits())):
            assert np.array_equal(a, b), f"step {k}, parameter {i}"
    assert buf.epoch_cursor() == (2, 0)
    assert all(not np.array_equal(a, b) for a, b in zip(start, cap.bits()))
    assert all(np.isfinite(_host_bits(p.detach()).view(np.float32)).all() for p in cap.params)
    eng.sync()
    eng.close()


# ---------------------------------------------------------------------------------------------- runtime guarantees
def test_no_host_synchronisation_no_allocation_and_untouched_state():
    """A condition, not a timing (as tests/test_minibatch.py checks minibatch): the stream is busy with milliseconds of fused steps
    before the calls and still busy when they have returned; with every output given torch's allocator hands out nothing; env state and
    the buffer's storage cursor are as they were, and the epoch cursor moved by exactly the three calls"""
    import torch
    from rl_ptg_amd import DeviceRolloutBuffer
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    n, T, calls, B = 65536, 250, 8, 256
    spec, _ = synthetic_spec(scenario=2, operation="OP2", eps_len_d=32)          # 4 608-step episodes: no boundary inside
    eng = HipEngine(spec.consts, spec.tables, spec.markets, n, device=0, out_dtype="float32", obs_layout="sb3_flat")
    eng.set_episode_plan(spec.eps_ind, n, n)
    eng.set_noise_rng(5)
    eng.reset()
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    acts = torch.randint(0, 5, (T, n), dtype=torch.int32, device="cuda", generator=g)
    obs, rew, done = eng.alloc_obs(T), torch.empty((T, n), device="cuda"), torch.empty((T, n), dtype=torch.uint8, device="cuda")
    buf = DeviceRolloutBuffer(eng, 2, seed=SEED)             # 131 072 rows, 512 batches of 256
    buf.actions.copy_(torch.arange(2 * n, device="cuda").view(n, 2).t())         # (t, e) holds e * T + t
    eng.rollout(acts, obs, rew, done)                        # warm: first-launch work is not part of the condition
    out = buf.next_batch(B)
    buf.end_epoch()
    buf.set_epoch_cursor(0, 510)
    torch.cuda.synchronize()
    cursor_before = buf.cursor()
    stream = torch.cuda.current_stream()
    assert stream.query() is True
    for _ in range(calls):
        eng.rollout(acts, obs, rew, done)
    busy_before = stream.query()
    allocs = torch.cuda.memory_stats()["allocation.all.allocated"]
    buf.next_batch(B, out=out)                               # (0, 510)
    buf.next_batch(B, out=out)                               # (0, 511), the epoch's last
    buf.next_batch(B, out=out)                               # (1, 0)
    buf.end_epoch()
    allocs_after = torch.cuda.memory_stats()["allocation.all.allocated"]
    busy_after = stream.query()
    assert busy_before is False, "the rollouts were over before the calls: the check would prove nothing"
    assert busy_after is False, "the stream was idle when the calls had returned: one of them waited for the device"
    assert allocs_after == allocs, "next_batch(out=...) or end_epoch allocated device memory"
    eng.sync()
    assert buf.epoch_cursor() == (2, 0) and buf.cursor() == cursor_before
    _same(out.actions, md.batch(2 * n, B, SEED, 1, 0))
    before = eng.state_dict()                                # the rollouts are over: what moves now, the calls moved
    buf.next_batch(B, out=out)
    buf.end_epoch()
    eng.sync()
    assert _equal_state(before, eng.state_dict()) and buf.cursor() == cursor_before and buf.epoch_cursor() == (3, 0)
    del obs, buf
    eng.close()


def test_a_side_stream():
    import torch
    T, N, B = 5, 13, 13
    eng = _engine(N, "sb3_flat", "mod", "float32")
    buf, host = _filled_buffer(eng, T, 11, np.random.default_rng(6))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert eng._stream().value == side.cuda_stream
        a = buf.next_batch(B)
        buf.end_epoch()
        b = buf.next_batch(B)
    side.synchronize()
    _check_batch(a, host, _order(T * N, 11, 0)[:B], "side stream")
    _check_batch(b, host, _order(T * N, 11, 1)[:B], "side stream, behind end_epoch")
    assert buf.epoch_cursor() == (1, 1)
    eng.sync()
    eng.close()


def test_refused_arguments_enqueue_nothing_and_a_valid_call_follows():
    import torch
    from rl_ptg_amd import _lib
    from rl_ptg_amd.engine import PtgError
    T, N, B = 6, 64, 48
    eng = _engine(N, "sb3_flat", "mod", "float32")
    F = eng.obs_dim
    rng = np.random.default_rng(13)
    x, c = _bits((T, N, F), 4, rng), _bits((T, N), 4, rng)
    obs, col = _fill_obs(eng, T, x), torch.from_numpy(c).cuda()
    cur = eng.new_epoch_cursor()
    out = torch.full((B, F), -777.25, dtype=torch.float32, device="cuda")
    out_c = torch.full((B,), -12345, dtype=torch.int32, device="cuda")
    io = torch.full((B,), -1, dtype=torch.int64, device="cuda")
    bad_out = lambda b: dict(obs_out=torch.empty((b, F), device="cuda"), columns_out=[torch.empty(b, dtype=torch.int32, device="cuda")],
                             idx_out=torch.empty(b, dtype=torch.int64, device="cuda"))
    b = dict(b50=bad_out(50), b768=bad_out(768), cur_f=cur.float(), cur_32=cur.int(), cur_1=torch.zeros(1, dtype=torch.int64, device="cuda"),
             cur_cpu=cur.cpu(), cur_st=torch.zeros(4, dtype=torch.int64, device="cuda")[::2], io_32=io.int(), io_f=io.double(), io_short=io[:B - 1],
             io_2d=io.view(B, 1), io_cpu=io.cpu())
    torch.cuda.synchronize()

    def untouched():
        assert torch.cuda.current_stream().query() is True
        assert bool((out == -777.25).all()) and bool((out_c == -12345).all()) and bool((io == -1).all()) and cur.tolist() == [0, 0]

    d = lambda **kw: eng.minibatch_drawn(kw.pop("cursor", cur), kw.pop("batch_size", B), obs, [col], obs_out=kw.pop("obs_out", out),
                                         columns_out=kw.pop("columns_out", [out_c]), idx_out=kw.pop("idx_out", io), **kw)
    refused = [
        (ValueError, lambda: d(batch_size=50, **b["b50"])),                              # 50 does not divide 384
        (ValueError, lambda: d(batch_size=768, **b["b768"])),                            # nor does twice the rollout
        (ValueError, lambda: d(batch_size=0)),
        (TypeError, lambda: d(cursor=None)),
        (TypeError, lambda: d(cursor=b["cur_f"])),
        (TypeError, lambda: d(cursor=b["cur_32"])),
        (TypeError, lambda: d(cursor=b["cur_1"])),
        (ValueError, lambda: d(cursor=b["cur_cpu"])),
        (ValueError, lambda: d(cursor=b["cur_st"])),
        (ValueError, lambda: d(idx_out=b["io_32"])),
        (ValueError, lambda: d(idx_out=b["io_f"])),
        (ValueError, lambda: d(idx_out=b["io_short"])),
        (ValueError, lambda: d(idx_out=b["io_2d"])),
        (ValueError, lambda: d(idx_out=b["io_cpu"])),
        (TypeError, lambda: eng.minibatch_end_epoch(None)),
        (TypeError, lambda: eng.minibatch_end_epoch(b["cur_f"])),
        (ValueError, lambda: eng.minibatch_end_epoch(b["cur_cpu"])),
    ]
    for exc, call in refused:
        with pytest.raises(exc):
            call()
        untouched()
    # the C entry points themselves
    L, h, st = eng._L, eng._h, eng._stream()
    vp = C.c_void_p
    arr = lambda *ptrs: (vp * len(ptrs))(*ptrs)

    def raw(handle=h, cu=cur.data_ptr(), i=io.data_ptr(), batch=B, T_=T, o=obs.data_ptr(), ob=4, dim=F, oo=out.data_ptr(), k=1, src=arr(col.data_ptr()),
            sz=(C.c_int32 * 1)(4), dst=arr(out_c.data_ptr()), s_t=N * F):
        return L.ptg_minibatch_drawn(handle, vp(cu) if cu else None, SEED, vp(i) if i else None, batch, T_, vp(o) if o else None, s_t, F, 1, dim, ob,
                                     vp(oo) if oo else None, k, src, sz, dst, st)

    bad = [dict(handle=None), dict(cu=None), dict(batch=50), dict(batch=5), dict(batch=2 * T * N), dict(batch=0), dict(batch=-4), dict(T_=0),
           dict(T_=-1), dict(T_=5), dict(ob=2), dict(dim=0), dict(s_t=-1), dict(o=None), dict(oo=None), dict(k=9), dict(k=-1), dict(src=None),
           dict(sz=None), dict(dst=None), dict(src=arr(None)), dict(dst=arr(None)), dict(sz=(C.c_int32 * 1)(3)), dict(o=None, oo=None, k=0)]
    for kw in bad:
        assert raw(**kw) == _lib.E_INVALID, kw
        if "handle" not in kw:
            assert b"ptg_minibatch_drawn" in L.ptg_last_error(h), kw
            with pytest.raises(PtgError):
                eng._chk(raw(**kw))
        untouched()
    assert L.ptg_minibatch_end_epoch(h, None, st) == _lib.E_INVALID and b"ptg_minibatch_end_epoch" in L.ptg_last_error(h)
    assert L.ptg_minibatch_end_epoch(None, vp(cur.data_ptr()), st) == _lib.E_INVALID
    untouched()
    # more rows than the bound: 2^18 envs x (2^31 - 1) steps; the batch divides them, nothing of that size exists, nothing is enqueued
    big = _engine(1 << 18, "sb3_flat", "mod", "float32")
    torch.cuda.synchronize()
    rc = big._L.ptg_minibatch_drawn(big._h, vp(cur.data_ptr()), 0, None, 1 << 18, 2 ** 31 - 1, None, 0, 0, 0, 0, 0, None, 1, arr(col.data_ptr()),
                                    (C.c_int32 * 1)(4), arr(out_c.data_ptr()), big._stream())
    assert rc == _lib.E_INVALID and b"2^48" in big._L.ptg_last_error(big._h)
    untouched()
    big.close()
    assert raw() == 0                                                                    # the same call with good arguments
    assert L.ptg_minibatch_end_epoch(h, vp(cur.data_ptr()), st) == 0
    eng.sync()
    exp = _order(T * N, SEED, 0)[:B]
    _same(io, np.array(exp)); _same(out, mr.gather(x, exp)); _same(out_c, mr.gather(c, exp))
    assert cur.tolist() == [1, 0]
    eng.close()
