"""ptg_rollout_buffer_begin / ptg_rollout_buffer_add, HipEngine.rollout_buffer_begin / rollout_buffer_add and
rl_ptg_amd.DeviceRolloutBuffer (include/ptg_env.h) -- the on-policy collect storage with its cursor on the device -- against the
row mapping that tests/rollout_buffer_restatement.py states and tests/test_rollout_buffer_host.py pins to SB3's RolloutBuffer.add /
reset (row t + 1 <- the new observation, row t of every column, nothing on overflow), applied here to a host mirror of the storage or
by a twin engine that stores with host indices; the window pipeline behind it against tests/gae_restatement.py / minibatch_restatement.py.

Every comparison is exact byte equality.  That is derived, not measured: the kernel copies.  Payloads are random BITS with NaN
payloads, infinities, signed zeros and subnormals planted, compared through integer views.  The storage of the raw-call tests lives
inside byte buffers filled with 0xA5, mirrored on the host: one comparison of the whole buffer covers the rows and columns not yet
added, the pad columns of a pitched feature-major block and the guard bytes around every allocation."""
import ctypes as C

import numpy as np
import pytest

import gae_restatement as gr
import minibatch_restatement as mr
from rl_ptg_amd.rollout_buffer import DeviceRolloutBuffer

pytestmark = pytest.mark.gpu

NS = [1, 63, 64, 65, 257]
FS = [16, 31, 40]                                            # float32 rows of 64, 124, 160 bytes; float64: 128, 248, 320
TS = [1, 2, 5]
SIZES = [4, 8]
LAYOUTS = ["row", "fm", "fm_pitch"]                          # [N][F]; [F][N] planes back to back; [F][N + 3]: planes at a pitch
SHIFTS = [(0, 0), (1, 0), (0, 1)]                            # elements by which (the rows' base, the source's base) miss 16-byte alignment
GUARD = 64                                                   # bytes before and behind every region
SENT = 0xA5
INT_OF = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}
SPECIAL32 = np.array([0x7FC00000, 0x7FC12345, 0xFFC00001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF], np.uint32)
SPECIAL64 = np.array([0x7FF8000000000000, 0x7FF8000000012345, 0xFFF8000000000001, 0x7FF0000000000000, 0xFFF0000000000000,
                      0x8000000000000000, 0x0000000000000001, 0x800FFFFFFFFFFFFF], np.uint64)

_specs = {}


def _tdt(size):
    import torch
    return {1: torch.uint8, 2: torch.int16, 4: torch.float32, 8: torch.float64}[size]


def _engine(n, layout="row", out_dtype="float32", **kw):
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    if "s" not in _specs:
        _specs["s"] = synthetic_spec(scenario=2, operation="OP2", eps_len_d=1, train_steps=200000)[0]      # 139-step episodes
    s = _specs["s"]
    eng = HipEngine(s.consts, s.tables, s.markets, n, device=0, out_dtype=out_dtype, obs_layout=layout, **kw)
    eng.set_episode_plan(s.eps_ind, n, n)
    eng.set_noise_rng(seed=4)
    return eng


def _bits(shape, itemsize, rng):
    a = rng.integers(0, 256, size=tuple(shape) + (itemsize,), dtype=np.uint8).view(INT_OF[itemsize])[..., 0].copy()
    if itemsize in (4, 8):
        sp = (SPECIAL32 if itemsize == 4 else SPECIAL64).view(INT_OF[itemsize])
        flat = a.reshape(-1)
        k = min(len(sp), flat.size)
        flat[:k] = sp[:k]
        flat[flat.size - k:] = sp[:k]
    return a


def _host_bits(t):
    import torch
    iv = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]
    return t.contiguous().view(iv).cpu().numpy()


def _same(got, exp, what=""):
    g = _host_bits(got)
    assert g.shape == exp.shape and g.itemsize == exp.itemsize, (what, g.shape, exp.shape, g.dtype, exp.dtype)
    np.testing.assert_array_equal(g, exp.view(g.dtype), err_msg=what)


class _Region:
    """`count` elements of `size` bytes inside a 0xA5 byte buffer on the device, `shift` elements behind a 16-byte boundary, guard
    bytes on both sides; `host` mirrors the whole buffer, `view` is the region in it"""

    def __init__(self, count, size, shift=0):
        import torch
        self.size, self.start = size, GUARD + shift * size
        self.raw = torch.full((self.start + count * size + GUARD,), SENT, dtype=torch.uint8, device="cuda")
        assert self.raw.data_ptr() % 16 == 0
        self.host = np.full(self.raw.numel(), SENT, np.uint8)
        self.view = self.host[self.start:self.start + count * size].view(INT_OF[size])
        self.ptr = self.raw.data_ptr() + self.start

    def put(self, a):
        """fill the region with the host integers a, on both sides"""
        import torch
        self.view[:] = a.reshape(-1)
        self.raw[self.start:self.start + a.size * self.size].copy_(torch.from_numpy(a.reshape(-1).view(np.uint8)))
        return self

    def check(self, what):
        got = self.raw.cpu().numpy()
        bad = np.nonzero(got != self.host)[0]
        assert bad.size == 0, (what, "first differing byte", int(bad[0]), "region", self.start, self.start + self.view.size * self.size)


def _block_elems(N, F, layout):
    return F * (N + 3) if layout == "fm_pitch" else N * F


def _strides(N, F, layout):
    """(obs_s_n, obs_s_f, row_pitch) of a block"""
    return {"row": (F, 1, N * F), "fm": (1, N, N * F), "fm_pitch": (1, N + 3, F * (N + 3))}[layout]


def _block_index(N, F, layout):
    """flat element index inside a block of env e, feature f, as an [N, F] array"""
    s_n, s_f, _ = _strides(N, F, layout)
    return np.arange(N)[:, None] * s_n + np.arange(F)[None, :] * s_f


class _Raw:
    """caller-owned storage described by a ptg_rollout_buffer and driven through the C entry points, with its host mirror"""

    def __init__(self, eng, T, F, size, layout, col_sizes, rng, shift=(0, 0), strided=()):
        from rl_ptg_amd import _lib
        self.eng, self.T, self.N, self.F, self.size, self.layout, self.col_sizes, self.rng = eng, T, eng.n, F, size, layout, list(col_sizes), rng
        self.strided = set(strided)                         # columns read at element stride 6, like out[:, 5] of a joint network output
        N = eng.n
        self.be = _block_elems(N, F, layout)
        self.rows = _Region((T + 1) * self.be, size, shift[0])
        self.src = _Region(self.be, size, shift[1])
        self.cols = [_Region(T * N, s) for s in col_sizes]
        self.cur = _Region(2, 8).put(np.array([3, 0], np.int64))                # begin must zero it
        self.idx = _block_index(N, F, layout).reshape(-1)
        self.pos = None
        d = _lib.PtgRolloutBuffer()
        d.n_steps, d.obs_dim, d.obs_bytes, d.obs_rows, d.n_cols, d.cursor_dev = T, F, size, self.rows.ptr, len(col_sizes), self.cur.ptr
        for c, (s, reg) in enumerate(zip(col_sizes, self.cols)):
            d.col_bytes[c], d.col_rows[c] = s, reg.ptr
        self.desc = d

    def _new_block(self):
        """a fresh source block: random bits everywhere, pad columns of a pitched block included (they must not travel)"""
        self.src.put(_bits((self.be,), self.size, self.rng))

    def _store(self, row):
        self.rows.view[row * self.be + self.idx] = self.src.view[self.idx]

    def begin(self):
        self._new_block()
        rc = self.eng._L.ptg_rollout_buffer_begin(self.eng._h, C.byref(self.desc), self.src.ptr, *_strides(self.N, self.F, self.layout), self.eng._stream())
        assert rc == 0, self.eng._L.ptg_last_error(self.eng._h)
        self._store(0)
        self.cur.view[:] = 0
        self.pos = 0

    def add(self, expect_stored=True):
        import torch
        self._new_block()
        k, N = len(self.col_sizes), self.N
        srcs, ptrs, strides = [], [], []
        for c, s in enumerate(self.col_sizes):
            w = 6 if c in self.strided else 1
            a = _bits((N, w), s, self.rng)
            t = torch.from_numpy(a).cuda()
            srcs.append((a[:, w - 1], t))
            ptrs.append(t.data_ptr() + (w - 1) * s)
            strides.append(w)
        rc = self.eng._L.ptg_rollout_buffer_add(self.eng._h, C.byref(self.desc), self.src.ptr, *_strides(N, self.F, self.layout), k,
                                                (C.c_void_p * max(k, 1))(*ptrs), (C.c_int64 * max(k, 1))(*strides), self.eng._stream())
        assert rc == 0, self.eng._L.ptg_last_error(self.eng._h)
        torch.cuda.synchronize()                            # the column sources die with this frame
        if expect_stored:
            self._store(self.pos + 1)
            for reg, (a, _) in zip(self.cols, srcs):
                reg.view[self.pos * N:(self.pos + 1) * N] = a
            self.pos += 1
            self.cur.view[0] = self.pos

    def check(self, what=""):
        import torch
        torch.cuda.synchronize()
        self.rows.check(what + " observation rows")
        for c, reg in enumerate(self.cols):
            reg.check(what + f" column {c}")
        self.cur.check(what + " cursor")


def _combos():
    """THE THINNING.  The full grid is N x F x T x element size x layout x alignment shift = 5 x 3 x 3 x 2 x 3 x 3.  Every N meets every
    (F, element size, layout) -- 18 cells per N -- while T and the alignment shift rotate diagonally through their lists, so that
    (checked below) every T and every shift still meets every F, every element size and every layout."""
    out = []
    for i, F in enumerate(FS):
        for j, size in enumerate(SIZES):
            for l, layout in enumerate(LAYOUTS):
                out.append((F, size, layout, TS[(i + j + l) % 3], SHIFTS[(i + 2 * j + 2 * l) % 3]))
    return out


def test_the_thinned_grid_meets_every_value_with_every_other():
    seen = set()
    for F, size, layout, T, shift in _combos():
        for a in (("F", F), ("size", size), ("layout", layout)):
            seen.add((a, ("T", T)))
            seen.add((a, ("shift", shift)))
    for a in [("F", f) for f in FS] + [("size", s) for s in SIZES] + [("layout", l) for l in LAYOUTS]:
        assert all((a, ("T", t)) in seen for t in TS), a
        assert all((a, ("shift", s)) in seen for s in SHIFTS), a
    assert len(_combos()) == 18


@pytest.mark.parametrize("N", NS)
def test_rows_columns_sentinels_and_cursor_after_every_add(N):
    """N at 1, around the wave and past one workgroup's 256 column lanes; F = 16, 40 through the 16-byte path when N * F * size and both
    bases allow it, F = 31 with an odd N and every shifted base through the element path, the pitched planes through the strided one;
    after begin and after EVERY add k <= T: rows > k of the observations, rows >= k of every column, pad columns and guard bytes keep
    0xA5, and the cursor reads {k, 0}"""
    eng = _engine(N)
    for q, (F, size, layout, T, shift) in enumerate(_combos()):
        rng = np.random.default_rng([N, F, size, T])
        col_sizes = [[8, 4, 4, 4, 1], [4, 1], [2, 8, 1]][q % 3]
        raw = _Raw(eng, T, F, size, layout, col_sizes, rng, shift, strided=[1] if q % 2 else [])
        what = f"N={N} F={F} size={size} {layout} T={T} shift={shift}"
        raw.begin()
        raw.check(what + " after begin")
        for k in range(1, T + 1):
            raw.add()
            raw.check(what + f" after add {k}")
    eng.close()


@pytest.mark.parametrize("n_cols", range(9))
def test_zero_to_eight_columns_of_every_element_size(n_cols):
    """columns of 1, 2, 4 and 8 bytes in rotating order, contiguous sources and sources read at stride 6 (out[:, 5])"""
    N, T, F = 65, 3, 40
    eng = _engine(N)
    sizes = [[1, 2, 4, 8, 8, 4, 2, 1][(c + n_cols) % 8] for c in range(n_cols)]
    for strided in ([], list(range(0, n_cols, 2)), list(range(n_cols))):
        raw = _Raw(eng, T, F, 4, "row", sizes, np.random.default_rng([n_cols, len(strided)]), strided=strided)
        raw.begin()
        for k in range(T):
            raw.add()
        raw.check(f"{n_cols} columns {sizes}, strided {strided}")
    eng.close()


def test_overflow_stores_nothing_and_begin_reopens_the_buffer():
    """the T + 1-th add changes no byte anywhere, leaves the cursor at {T, 0} and makes sync() raise PTG_E_INDEX exactly once; after
    begin() the buffer fills again"""
    from rl_ptg_amd import _lib
    from rl_ptg_amd.engine import PtgError
    N, T, F = 65, 2, 40
    eng = _engine(N)
    for layout, size in (("row", 4), ("fm_pitch", 8)):
        raw = _Raw(eng, T, F, size, layout, [4, 1], np.random.default_rng(11), strided=[0])
        raw.begin()
        raw.add(); raw.add()
        raw.check("full")
        eng.sync()                                          # nothing pending
        raw.add(expect_stored=False)
        raw.check("after the add on a full buffer")
        assert raw.cur.view.tolist() == [T, 0]
        with pytest.raises(PtgError) as ei:
            eng.sync()
        assert ei.value.code == _lib.E_INDEX and "ptg_rollout_buffer_add" in str(ei.value)
        eng.sync()                                          # reported once
        raw.add(expect_stored=False)                        # and again: still nothing
        raw.check("after the second add on a full buffer")
        with pytest.raises(PtgError):
            eng.sync()
        raw.begin()
        raw.check("reopened")
        raw.add(); raw.add()
        raw.check("refilled")
        eng.sync()
    eng.close()


def _equal_state(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_equal_state(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return a == b


class _Twin:
    """a second engine running the same collect step eagerly, storing with host indices into plain tensors"""

    def __init__(self, eng, pi, T, seed):
        import torch
        from rl_ptg_amd import DeviceMLP
        self.eng, self.T, self.seed = eng, T, seed
        self.policy = DeviceMLP(eng, pi, batch=eng.n)
        self.counter = eng.new_draw_counter()
        N = eng.n
        self.rows = eng.alloc_obs(T + 1, zero=True)
        z = lambda dt: torch.zeros((T, N), dtype=dt, device="cuda")
        self.actions, self.values, self.log_probs, self.rewards, self.dones = z(torch.int64), z(torch.float32), z(torch.float32), z(torch.float32), z(torch.uint8)

    def window(self):
        eng = self.eng
        self.rows[0].copy_(eng.obs)
        for t in range(self.T):
            out = self.policy(eng.obs)
            head = eng.act_categorical(out[:, :5], self.counter, seed=self.seed, act_dtype=self.actions.dtype)
            self.values[t].copy_(out[:, 5])
            eng.step(head.actions)
            self.rows[t + 1].copy_(eng.obs)
            for ring, x in ((self.actions, head.actions), (self.log_probs, head.log_prob), (self.rewards, eng.rew), (self.dones, eng.done)):
                ring[t].copy_(x)
        eng.sync()


def _check_window(buf, twin, policy, what):
    """every byte of the buffer equals the twin's; then the window pipeline: compute_returns_and_advantage and get(batch_size=7) against
    the restatements, bit for bit"""
    import torch
    eng, T, N = buf.engine, buf.n_steps, buf.n_envs
    eng.sync()
    assert buf.cursor() == (T, 0) and buf.full and buf.pos == T
    assert torch.equal(buf.storage.obs_rows.view(torch.int32), twin.rows.view(torch.int32)), what + " observation rows"
    for name in buf.names:
        _same(buf.column(name), _host_bits(getattr(twin, name)), what + " " + name)
    assert torch.equal(buf.last_obs, eng.obs) and buf.observations.shape == (T, N, eng.obs_dim)
    last_values = policy(buf.last_obs)[:, 5].contiguous()
    adv, ret = buf.compute_returns_and_advantage(last_values, 0.97, 0.9)
    assert adv.data_ptr() == buf.advantages.data_ptr() and ret.data_ptr() == buf.returns.data_ptr()
    eng.sync()
    h = lambda t: t.cpu().numpy()
    e_adv, e_ret = gr.gae(h(twin.rewards), h(twin.values), h(twin.dones), h(last_values), 0.97, 0.9, np.float32)
    _same(buf.advantages, e_adv.view(np.int32), what + " advantages")
    _same(buf.returns, e_ret.view(np.int32), what + " returns")
    perm = torch.randperm(T * N, device="cuda")
    got = list(buf.get(batch_size=7, perm=perm))
    eng.sync()
    exp = list(mr.minibatches(h(perm), 7, obs=h(twin.rows[:T]), columns=[h(twin.actions), h(twin.values), h(twin.log_probs), e_adv, e_ret]))
    assert len(got) == len(exp) == -(-T * N // 7)
    for b, (g, (eo, ecols)) in enumerate(zip(got, exp)):
        _same(g.observations, eo.view(np.int32), what + f" batch {b} observations")
        for field, e in zip(g[1:], ecols):
            _same(field, e.view(INT_OF[e.itemsize]), what + f" batch {b}")
    one = list(buf.get())                                   # A2C: one batch of everything, its own permutation
    assert len(one) == 1 and one[0].observations.shape == (T * N, eng.obs_dim) and one[0].returns.shape == (T * N,)
    return int(twin.dones.sum())


def test_captured_collect_step_and_the_window_pipeline():
    """DeviceMLP 40 -> 37 -> 5 + a value column -> act_categorical -> replay-proof step -> add at 64 envs, captured on a side stream at
    the default hardware-queue setting.  Row 0 is begin's, row 1 the eager call's before the capture (capturing runs nothing: the cursor
    proves it), rows 2 .. T = 5 the replays', across the episode end on step 139.  Every buffer byte equals a twin engine's eager loop
    that stores with host indices; engine state too.  Then compute_returns_and_advantage and get(batch_size=7) against the
    restatements, and a second window after begin(), all five rows by replays."""
    import torch
    from torch import nn
    from rl_ptg_amd import DeviceMLP
    N, T, PRE, SEED = 64, 5, 136, 3
    eng, twin_eng = _engine(N, "sb3_flat"), _engine(N, "sb3_flat")
    torch.manual_seed(5)
    pi = nn.Sequential(nn.Linear(40, 37), nn.Tanh(), nn.Linear(37, 6)).cuda()
    g = torch.Generator(device="cuda"); g.manual_seed(6)
    pre = torch.randint(0, 5, (PRE, N), dtype=torch.int32, device="cuda", generator=g)
    for e in (eng, twin_eng):
        e.vn_init()
        e.set_replay_proof(True)
        e.reset()
        o, _, _ = e.rollout(pre)                            # 136 of the episode's 139 steps: the window crosses its end
        e.obs.copy_(o[-1])
    twin = _Twin(twin_eng, pi, T, SEED)
    policy = DeviceMLP(eng, pi, batch=N)
    counter = eng.new_draw_counter()
    buf = DeviceRolloutBuffer(eng, T)
    out = policy(eng.obs)
    head = eng.act_categorical(out[:, :5], counter, seed=SEED, act_dtype=torch.int64)
    counter.zero_()                                         # that call only made the static outputs

    def one():
        out = policy(eng.obs)
        eng.act_categorical(out[:, :5], counter, seed=SEED, out=head)
        eng.step(head.actions)
        buf.add(eng.obs, eng.rew, eng.done, actions=head.actions, values=out[:, 5], log_probs=head.log_prob)

    buf.begin()
    one()                                                   # eager once: code objects are loaded before the capture
    eng.sync()
    assert buf.cursor() == (1, 0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            one()
    torch.cuda.current_stream().wait_stream(side)
    assert buf.cursor() == (1, 0)                           # capturing enqueued nothing
    for k in range(2, T + 1):
        graph.replay()
        torch.cuda.synchronize()
        assert buf.cursor() == (k, 0)
    eng.note_replays(T - 1 - 1)                             # T - 1 replays; the capture call counted as one step on the host
    twin.window()
    ended = _check_window(buf, twin, policy, "window 1")
    assert ended == N, ended                                # the episode end lay inside the window
    a, b = eng.state_dict(), twin_eng.state_dict()
    assert _equal_state(a["fields"], b["fields"]) and _equal_state(a["vn"], b["vn"])
    # the second window: begin() takes this window's new_obs, then T replays of the same graph
    buf.begin()
    eng.sync()
    assert buf.cursor() == (0, 0) and torch.equal(buf.storage.obs_rows[0], buf.storage.obs_rows[T])
    for k in range(1, T + 1):
        graph.replay()
    torch.cuda.synchronize()
    eng.note_replays(T)
    twin.window()
    _check_window(buf, twin, policy, "window 2")
    a, b = eng.state_dict(), twin_eng.state_dict()
    assert _equal_state(a["fields"], b["fields"]) and _equal_state(a["vn"], b["vn"])
    assert len(eng.finished_episodes()[0]) == len(twin_eng.finished_episodes()[0])
    eng.close(); twin_eng.close()


@pytest.mark.parametrize("layout,kw", [("split", {}), ("feature", {}), ("feature", {"obs_pitch": 73})])
def test_an_eager_collect_loop_in_every_engine_layout(layout, kw):
    """DeviceRolloutBuffer behind step() in the split (F = 16) and feature-major layouts, with and without a pitch, float64 rewards and
    observations in the pitched case; a strided value source; the buffer's rows equal copies made with host indices and minibatches
    gather from them"""
    import torch
    N, T = 65, 4
    eng = _engine(N, layout, "float64" if kw else "float32", **kw)
    buf = DeviceRolloutBuffer(eng, T, columns={"actions": torch.int32, "values": torch.float64})
    g = torch.Generator(device="cuda"); g.manual_seed(7)
    acts = torch.randint(0, 5, (T, N), dtype=torch.int32, device="cuda", generator=g)
    out = torch.randn((T, N, 6), dtype=torch.float64, device="cuda", generator=g)
    rows = eng.alloc_obs(T + 1, zero=True)
    rews, dones = torch.zeros((T, N), dtype=eng.out_dtype, device="cuda"), torch.zeros((T, N), dtype=torch.uint8, device="cuda")
    eng.reset()
    buf.begin()
    rows[0].copy_(eng.obs)
    for t in range(T):
        obs, rew, done = eng.step(acts[t])
        buf.add(obs, rew, done, actions=acts[t], values=out[t, :, 5])
        rows[t + 1].copy_(obs); rews[t].copy_(rew); dones[t].copy_(done)
    eng.sync()
    assert buf.cursor() == (T, 0)
    _same(eng.rows(buf.storage.obs_rows), _host_bits(eng.rows(rows)), "rows")
    if kw:                                                  # the pad columns of the zeroed storage stayed zero
        full = buf.storage.obs_rows.as_strided((T + 1, eng.obs_dim, eng.pitch), (eng.obs_dim * eng.pitch, eng.pitch, 1))
        assert int(torch.count_nonzero(full[..., N:])) == 0
    for name, exp in (("actions", acts), ("values", out[:, :, 5]), ("rewards", rews), ("dones", dones)):
        _same(buf.column(name), _host_bits(exp), name)
    perm = torch.randperm(T * N, device="cuda", generator=g)
    o, (a,) = next(iter(eng.minibatches(perm, 50, obs=buf.observations, columns=[buf.actions])))
    eng.sync()
    idx = perm[:50].cpu().numpy()
    _same(o, mr.gather(_host_bits(eng.rows(rows[:T])), idx))
    _same(a, mr.gather(_host_bits(acts), idx))
    eng.close()


def test_no_host_synchronisation_and_no_allocation_at_65536_envs():
    """A condition, not a timing (as tests/test_replay.py checks replay_add): the stream is busy with milliseconds of fused steps
    before begin / add and still busy when they have returned; torch's allocator hands out nothing in between"""
    import torch
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    n, T, calls = 65536, 250, 8
    spec, _ = synthetic_spec(scenario=2, operation="OP2", eps_len_d=32)          # 4 608-step episodes: no boundary inside
    eng = HipEngine(spec.consts, spec.tables, spec.markets, n, device=0, out_dtype="float32", obs_layout="sb3_flat")
    eng.set_episode_plan(spec.eps_ind, n, n)
    eng.set_noise_rng(5)
    eng.reset()
    buf = DeviceRolloutBuffer(eng, 3, columns={"actions": torch.int32})
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    acts = torch.randint(0, 5, (T, n), dtype=torch.int32, device="cuda", generator=g)
    obs, rew, done = eng.alloc_obs(T), torch.empty((T, n), dtype=torch.float32, device="cuda"), torch.empty((T, n), dtype=torch.uint8, device="cuda")
    eng.rollout(acts, obs, rew, done)                                        # warm: first-launch work is not part of the condition
    buf.begin(obs[0])
    buf.add(obs[1], rew[1], done[1], actions=acts[1])
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    assert stream.query() is True
    for _ in range(calls):
        eng.rollout(acts, obs, rew, done)
    busy_before = stream.query()
    allocated = torch.cuda.memory_allocated()
    buf.begin(obs[2])
    buf.add(obs[3], rew[3], done[3], actions=acts[3])
    buf.add(obs[4], rew[4], done[4], actions=acts[4])
    grown = torch.cuda.memory_allocated() - allocated
    busy_after = stream.query()
    assert busy_before is False, "the rollouts were over before the calls: the check would prove nothing"
    assert busy_after is False, "the stream was idle when begin and add had returned: a call waited for the device"
    assert grown == 0, f"{grown} bytes allocated across begin / add"
    eng.sync()
    assert buf.cursor() == (2, 0) and not buf.full
    rows = buf.storage.obs_rows
    assert torch.equal(rows[0], obs[2]) and torch.equal(rows[1], obs[3]) and torch.equal(rows[2], obs[4]) and int(torch.count_nonzero(rows[3])) == 0
    assert torch.equal(buf.actions[:2], acts[3:5]) and torch.equal(buf.rewards[:2], rew[3:5]) and torch.equal(buf.dones[:2], done[3:5])
    assert int(torch.count_nonzero(buf.actions[2])) == 0
    del buf, rows
    eng.close()


def test_a_side_stream_and_two_runs_with_identical_bytes():
    import torch
    N, T, F = 257, 5, 40
    eng = _engine(N)
    side = torch.cuda.Stream()
    snaps = []
    for run in range(2):
        raw = _Raw(eng, T, F, 4, "row", [8, 4, 1], np.random.default_rng(21), strided=[1])
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            assert eng._stream().value == side.cuda_stream
            raw.begin()
            for k in range(T):
                raw.add()
        raw.check(f"run {run} on a side stream")
        snaps.append([raw.rows.raw.cpu().numpy()] + [c.raw.cpu().numpy() for c in raw.cols] + [raw.cur.raw.cpu().numpy()])
    assert all(np.array_equal(a, b) for a, b in zip(*snaps))
    eng.close()


def test_refused_descriptors_enqueue_nothing_and_a_valid_call_follows():
    import torch
    from rl_ptg_amd import _lib
    N, T, F = 64, 3, 40
    eng = _engine(N)
    raw = _Raw(eng, T, F, 4, "row", [8, 4], np.random.default_rng(8))
    raw.begin()
    raw.add()
    raw.check()
    L, h, stream = eng._L, eng._h, eng._stream()
    vp = C.c_void_p
    col8, col4 = torch.zeros(N, dtype=torch.float64, device="cuda"), torch.zeros(N, device="cuda")
    arr = lambda *ptrs: (vp * len(ptrs))(*ptrs)
    i64 = lambda *v: (C.c_int64 * len(v))(*v)
    torch.cuda.synchronize()

    def desc(**kw):
        d = _lib.PtgRolloutBuffer.from_buffer_copy(raw.desc)
        for k, v in kw.items():
            if k in ("col_bytes", "col_rows"):
                getattr(d, k)[v[0]] = v[1]
            else:
                setattr(d, k, v)
        return d

    def raw_add(d=None, handle=h, o=raw.src.ptr, s_n=F, s_f=1, pitch=N * F, k=2, src=arr(col8.data_ptr(), col4.data_ptr()), st=i64(1, 1)):
        d = desc() if d is None else d
        return L.ptg_rollout_buffer_add(handle, C.byref(d) if d != "null" else None, o, s_n, s_f, pitch, k, src, st, stream)

    def raw_begin(d=None, handle=h, o=raw.src.ptr, s_n=F, s_f=1, pitch=N * F):
        d = desc() if d is None else d
        return L.ptg_rollout_buffer_begin(handle, C.byref(d) if d != "null" else None, o, s_n, s_f, pitch, stream)

    def nothing_happened(what):
        assert torch.cuda.current_stream().query() is True, what
        raw.check(str(what))

    bad_desc = [dict(n_steps=0), dict(n_steps=-3), dict(obs_dim=0), dict(obs_dim=(1 << 20) + 1), dict(obs_bytes=2), dict(obs_bytes=16), dict(obs_rows=None),
                dict(cursor_dev=None), dict(n_cols=9), dict(n_cols=-1), dict(col_bytes=(0, 3)), dict(col_bytes=(1, 16)), dict(col_bytes=(1, 0)), dict(col_rows=(1, None))]
    bad_both = [dict(d="null"), dict(handle=None), dict(o=None), dict(s_n=-1), dict(s_f=-1), dict(pitch=-1)] + [dict(d=desc(**kw)) for kw in bad_desc]
    bad_add = bad_both + [dict(k=1), dict(k=3), dict(k=-1), dict(k=9), dict(src=None), dict(st=None), dict(src=arr(None, col4.data_ptr())), dict(src=arr(col8.data_ptr(), None)),
                          dict(st=i64(0, 1)), dict(st=i64(1, -6)), dict(d=desc(n_cols=1)), dict(d=desc(n_cols=3, col_bytes=(2, 4), col_rows=(2, raw.cols[1].ptr)))]
    for fn, name, bad in ((raw_add, b"ptg_rollout_buffer_add", bad_add), (raw_begin, b"ptg_rollout_buffer_begin", bad_both)):
        for kw in bad:
            assert fn(**kw) == _lib.E_INVALID, (name, kw)
            if "handle" not in kw:
                assert name in L.ptg_last_error(h), (name, kw, L.ptg_last_error(h))
            nothing_happened((name, {k: v for k, v in kw.items() if k != "d"}))
    raw.add()                                                # the same call with good arguments
    raw.check("the valid call after the refusals")
    assert raw.cur.view.tolist() == [2, 0]
    eng.sync()
    eng.close()
