"""ptg_replay_add / ptg_replay_sample, HipEngine.replay_add / replay_sample and rl_ptg_amd.DeviceReplayBuffer (include/ptg_env.h) --
the replay buffer of the off-policy algorithms on the device -- against the NumPy restatement of SB3's ReplayBuffer and of the
device index draw (tests/replay_restatement.py, pinned by tests/test_replay_host.py).

Every comparison is exact byte equality.  That is derived, not measured: the kernels copy (the done column is a 0.0f / 1.0f select
and the normalised reward is k_vn_norm's expression, compared with that kernel's own output).  Payloads are random BITS with NaN
payloads, infinities, signed zeros and subnormals planted, compared through integer views."""
import ctypes as C

import numpy as np
import pytest

import replay_restatement as rr

pytestmark = pytest.mark.gpu

NS = [1, 6, 63, 64, 65, 200]
SS = [1, 2, 5, 7]
FS = [1, 3, 4, 35, 40]                                       # float32: 4, 12, 16, 140, 160-byte rows; float64: 8, 24, 32, 280, 320
SIZES = [4, 8]
SOURCES = ["row", "fm", "fm_pitch"]
BS = [1, 15, 16, 17, 64 * 4 * 16 + 1]
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


def _dev(a):
    """host integer array -> device tensor of the float (4, 8 bytes) or integer (1, 2) dtype of that size, same bits"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().view(_tdt(a.itemsize))


def _host_bits(t):
    import torch
    iv = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]
    return t.contiguous().view(iv).cpu().numpy()


def _same(got, exp, what=""):
    g = _host_bits(got)
    assert g.shape == exp.shape and g.itemsize == exp.itemsize, (what, g.shape, exp.shape, g.dtype, exp.dtype)
    np.testing.assert_array_equal(g, exp.view(g.dtype), err_msg=what)


def _rows_view(x, source):
    """device ROW VIEW [..., N, F] of the host bits x, stored row-major, feature-major [..., F, N] or feature-major with pitch N + 3"""
    import torch
    if source == "row":
        return _dev(x)
    xt = np.ascontiguousarray(np.swapaxes(x, -1, -2))
    if source == "fm":
        return _dev(xt).transpose(-1, -2)
    pad = torch.zeros(xt.shape[:-1] + (xt.shape[-1] + 3,), dtype=_tdt(x.itemsize), device="cuda")
    pad[..., :xt.shape[-1]].copy_(_dev(xt))
    return pad[..., :xt.shape[-1]].transpose(-1, -2)


def _clone(eng, x):
    """a copy of an [N, F] / [F, N] observation in the engine's own layout (clone() would drop a feature-major pitch)"""
    y = eng.alloc_obs()
    y.copy_(x)
    return y


def _storage(S, N, F, size, col_sizes):
    import torch
    from rl_ptg_amd.replay import ReplayStorage
    z = lambda shape, s: torch.zeros(shape, dtype=_tdt(s), device="cuda")
    return ReplayStorage(z((S, N, F), size), z((S, N, F), size), [z((S, N), s) for s in col_sizes], torch.zeros(2, dtype=torch.int64, device="cuda"))


class _Pair:
    """a device storage and the restatement, fed the same windows"""

    def __init__(self, eng, S, F, size, col_sizes, done_col, rng):
        self.eng, self.S, self.N, self.F, self.size, self.col_sizes, self.done_col, self.rng = eng, S, eng.n, F, size, col_sizes, done_col, rng
        self.st = _storage(S, eng.n, F, size, col_sizes)
        self.ref = rr.ReplayBuffer(S * eng.n, eng.n, F, INT_OF[size], [INT_OF[s] for s in col_sizes])
        assert self.ref.buffer_size == S
        self.last = _bits((eng.n, F), size, rng)
        self.added = 0

    def window(self, T):
        rng = self.rng
        x, fin = _bits((T, self.N, self.F), self.size, rng), _bits((T, self.N, self.F), self.size, rng)
        done = (rng.random((T, self.N)) < 0.35).astype(np.uint8) * rng.integers(1, 256, (T, self.N)).astype(np.uint8)      # any non-zero byte is "done"
        cols = [None if c == self.done_col else _bits((T, self.N), s, rng) for c, s in enumerate(self.col_sizes)]
        return x, fin, done, cols

    def add(self, T, source="row", with_fin=True):
        x, fin, done, cols = self.window(T)
        self.eng.replay_add(self.st, _rows_view(self.last, source), _rows_view(x, source), [None if c is None else _dev(c) for c in cols],
                            done=_dev(done), final_obs=_rows_view(fin, source) if with_fin else None, done_col=self.done_col)
        rr.store_window(self.ref, self.last, x, done, cols, fin if with_fin else None, self.done_col if self.done_col >= 0 else None)
        self.last = x[-1]
        self.added += T

    def check(self, what=""):
        self.eng.sync()
        _same(self.st.obs_ring, self.ref.observations, what + " observations")
        _same(self.st.next_ring, self.ref.next_observations, what + " next observations")
        for c, (ring, exp) in enumerate(zip(self.st.col_rings, self.ref.columns)):
            _same(ring, exp, what + f" column {c}")
        assert self.st.cursor.cpu().tolist()[0] == self.added
        assert (self.added % self.S, self.added >= self.S, min(self.added, self.S)) == (self.ref.pos, self.ref.full, self.ref.size())

    def check_sample(self, idx, what="", **kw):
        import torch
        o, n, outs, io = self.eng.replay_sample(self.st, idx=torch.from_numpy(np.asarray(idx, np.int64)).cuda(), want_idx=True, **kw)
        self.eng.sync()
        eo, en, ecols = self.ref.get_flat(idx)
        _same(o, eo, what + " sampled observations"); _same(n, en, what + " sampled next observations")
        for c, (got, exp) in enumerate(zip(outs, ecols)):
            _same(got, exp, what + f" sampled column {c}")
        assert np.array_equal(io.cpu().numpy(), np.asarray(idx, np.int64))


def _combos():
    """every (S, F, element size) once, source layout, final_obs and B rotating through their lists"""
    out = []
    for i, S in enumerate(SS):
        for j, F in enumerate(FS):
            for k, size in enumerate(SIZES):
                q = 10 * i + 2 * j + k
                out.append((S, F, size, SOURCES[q % 3], q % 4 != 3, BS[(i + j + k) % 5]))
    return out


def test_the_combinations_meet_every_value_with_every_source():
    seen = {(key, v, src) for S, F, size, src, fin, B in _combos() for key, v in (("S", S), ("F", F), ("size", size), ("B", B))}
    want = [("S", s) for s in SS] + [("F", f) for f in FS] + [("size", s) for s in SIZES] + [("B", b) for b in BS]
    assert all((k, v, src) in seen for k, v in want for src in SOURCES if k != "B")
    assert all(any((k, v, src) in seen for src in SOURCES) for k, v in want)
    assert {fin for *_, fin, _ in _combos()} == {True, False}


@pytest.mark.parametrize("N", NS)
def test_windows_rows_and_sources(N):
    """N at 1, around the wave and past one tile of 64 envs; S, T in {1, 3, S}, F and element size through the 16-byte path (16-,
    160-, 32-, 280-, 320-byte rows ...) and the element path; row-major and feature-major sources, with and without a pitch;
    windows that wrap mid-way and many adds past `full`; with and without final_obs; a float32 done column and 1-, 2-, 8-byte
    columns; then explicit-index samples of B rows with repeats"""
    eng = _engine(N)
    for S, F, size, source, with_fin, B in _combos():
        rng = np.random.default_rng([N, S, F, size])
        pair = _Pair(eng, S, F, size, [8, 4, 1, 2], 1, rng)
        what = f"N={N} S={S} F={F} size={size} {source} final_obs={with_fin}"
        for T in [1, min(3, S), S, 1, min(3, S), S, S, 1]:  # S = 5: positions 1, 4, then a T = 5 window wrapping mid-way, ...
            pair.add(T, source, with_fin)
        pair.check(what)
        assert pair.ref.full
        idx = rng.integers(0, S * N, B)
        pair.check_sample(idx, what + f" B={B}")
    eng.close()


def test_partly_filled_buffer_and_every_sample_size():
    """size < S: only the live rows are legal; B in {1, 15, 16, 17, 4 097} with and without repeats; only some outputs asked for"""
    import torch
    N, S, F = 65, 7, 40
    eng = _engine(N)
    pair = _Pair(eng, S, F, 4, [4, 4], 1, np.random.default_rng(2))
    pair.add(3); pair.add(1)
    pair.check("4 of 7 rows")
    assert pair.ref.size() == 4 and not pair.ref.full
    rng = np.random.default_rng(3)
    for B in BS:
        pair.check_sample(rng.integers(0, 4 * N, B), f"B={B}")
    pair.check_sample(np.full(33, 4 * N - 1), "one index 33 times")
    pair.check_sample(rng.permutation(4 * N), "a permutation of everything")
    idx = rng.integers(0, 4 * N, 50)
    idx_d = torch.from_numpy(idx).cuda()
    eo, en, ecols = pair.ref.get_flat(idx)
    o, n, outs, io = eng.replay_sample(pair.st, idx=idx_d, want_obs=False, want_cols=[False, True])
    eng.sync()
    assert o is None and outs[0] is None and io is None
    _same(n, en); _same(outs[1], ecols[1])
    o, n, outs, io = eng.replay_sample(pair.st, idx=idx_d, want_next=False, want_cols=[False, False])
    eng.sync()
    assert n is None and outs == [None, None]
    _same(o, eo)
    eng.close()


def test_byte_offsets_past_4_gib():
    """float32 rings [412, 65 536, 40] are 4 320 133 120 bytes each, past 2^32; the cursor is placed on the last row of a full buffer,
    so a 2-step window goes to the last row (byte offset 4.3e9) and wraps to row 0; element values are their own index in the window"""
    import torch
    from rl_ptg_amd.replay import ReplayStorage
    N, F, S = 65536, 40, 412
    free = torch.cuda.mem_get_info()[0]
    if free < 12 * 2 ** 30:
        print(f"test_byte_offsets_past_4_gib skipped: {free / 2 ** 30:.2f} GiB of device memory free, 12 GiB needed")
        pytest.skip(f"{free / 2 ** 30:.2f} GiB of device memory free, 12 GiB needed")
    eng = _engine(N, "sb3_flat")
    assert (S - 1) * N * F * 4 > 2 ** 32
    st = ReplayStorage(torch.zeros((S, N, F), device="cuda"), torch.zeros((S, N, F), device="cuda"), [torch.zeros((S, N), dtype=torch.int32, device="cuda")],
                       torch.tensor([2 * S - 1, 0], dtype=torch.int64, device="cuda"))
    x = torch.arange(2 * N * F, dtype=torch.int32, device="cuda").view(2, N, F)
    prev = -torch.arange(1, N * F + 1, dtype=torch.int32, device="cuda").view(N, F)
    col = torch.arange(2 * N, dtype=torch.int32, device="cuda").view(2, N) + 7
    eng.replay_add(st, prev.view(torch.float32), x.view(torch.float32), [col])
    rng = np.random.default_rng(10)
    e = np.concatenate([[0, N - 1], rng.integers(0, N, 98)])
    idx = np.concatenate([(S - 1) * N + e, e])               # the last row, then row 0
    o, n, (c,), _ = eng.replay_sample(st, idx=torch.from_numpy(idx).cuda())
    eng.sync()
    assert st.cursor.cpu().tolist() == [2 * S + 1, 0]
    f = np.arange(F)[None, :]
    row = lambda t, e: ((t * N + e)[:, None] * F + f).astype(np.int32)
    zero = np.zeros_like(e)
    _same(o, np.concatenate([-(row(zero, e) + 1), row(zero, e)]))           # the last row holds prev, row 0 the window's step 0
    _same(n, np.concatenate([row(zero, e), row(zero + 1, e)]))
    _same(c, np.concatenate([e + 7, N + e + 7]).astype(np.int32))
    assert int(torch.count_nonzero(st.obs_ring[1:S - 1])) == 0 and int(torch.count_nonzero(st.next_ring[1:S - 1])) == 0      # nothing strayed in between
    del st, o, n
    eng.close()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("layout,F", [("split", 16), ("sb3_flat", 40), ("feature", 35)])
def test_a_real_collect_loop_across_an_episode_end(layout, F):
    """DeviceReplayBuffer behind a discrete-action step() loop of 150 steps on 139-step episodes, N = 6, a buffer of 40 rows (so it
    wraps three times): equal to the restatement fed the same step outputs, final_obs in place on the episode's last step"""
    import torch
    from rl_ptg_amd import DeviceReplayBuffer
    N, K = 6, 150
    eng = _engine(N, layout, obs_pitch=8 if layout == "feature" else None)
    assert eng.obs_dim == F
    buf = DeviceReplayBuffer(eng, 40 * N + 5, columns={"actions": torch.int32, "log_prob": torch.float64}, seed=9)
    assert buf.buffer_size == 40 and buf.size() == 0
    ref = rr.ReplayBuffer(40 * N + 5, N, F, np.int32, [np.int32, np.int64, np.int32, np.int32])
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    acts = torch.randint(0, 5, (K, N), dtype=torch.int32, device="cuda", generator=g)
    logp = torch.randn((K, N), dtype=torch.float64, device="cuda", generator=g)
    prev = _clone(eng, eng.reset())
    rec, n_done = [], 0
    for t in range(K):
        obs, rew, done = eng.step(acts[t])
        buf.add(prev, obs, rew, done, final_obs=eng.final_obs, actions=acts[t], log_prob=logp[t])
        rec.append([_host_bits(eng.rows(x).contiguous()) for x in (prev, obs, eng.final_obs)] + [_host_bits(rew), done.cpu().numpy()])
        prev = _clone(eng, obs)
        n_done += int(done.sum())
    eng.sync()
    assert n_done == N                                       # the episodes ended inside the loop
    for t, (p, o, f, r, d) in enumerate(rec):
        rr.store_window(ref, p, o[None], d[None], [_host_bits(acts[t])[None], _host_bits(logp[t])[None], r[None], None], f[None], done_col=3)
    assert (buf.pos, buf.full, buf.size()) == (ref.pos, ref.full, ref.size()) == (K % 40, True, 40)
    _same(buf.observations, ref.observations); _same(buf.next_observations, ref.next_observations)
    for name, exp in zip(buf.names, ref.columns):
        _same(buf.column(name), exp, name)
    d_ring = buf.column("dones").cpu().numpy()
    assert d_ring.dtype == np.float32 and d_ring.sum() == N and set(np.unique(d_ring)) == {0.0, 1.0}
    slot = int(np.nonzero(d_ring[:, 0])[0][0])
    t_end = [t for t, r in enumerate(rec) if r[4].any()][0]
    assert np.array_equal(_host_bits(buf.next_observations[slot]), rec[t_end][2])           # the terminal observation ...
    assert not np.array_equal(rec[t_end][2], rec[t_end][1])                                 # ... which is not the post-reset one
    idx = torch.randint(0, 40 * N, (203,), device="cuda", generator=g)
    s, extra = buf.sample(idx=idx, extras=True)
    eng.sync()
    eo, en, ecols = ref.get_flat(idx.cpu().numpy())
    assert s.observations.shape == (203, F) and s.actions.shape == s.dones.shape == s.rewards.shape == (203, 1) and s.dones.dtype == torch.float32
    _same(s.observations, eo); _same(s.next_observations, en)
    for got, exp in zip((s.actions, extra["log_prob"], s.rewards, s.dones), ecols):
        _same(got[:, 0], exp)
    eng.close()


def test_a_rollout_window_and_the_state_dict_round_trip():
    """[T, N] windows from rollout() through DeviceReplayBuffer.add (no final_obs: the post-reset observation stays), then
    state_dict() -> a fresh buffer -> load_state_dict(): the same rings, position and next device-drawn batch"""
    import torch
    from rl_ptg_amd import DeviceReplayBuffer
    N, T = 65, 20
    eng = _engine(N, "sb3_flat")
    buf = DeviceReplayBuffer(eng, 50 * N, seed=21)
    ref = rr.ReplayBuffer(50 * N, N, 40, np.int32, [np.int64, np.int32, np.int32])
    g = torch.Generator(device="cuda"); g.manual_seed(2)
    prev = _clone(eng, eng.reset())
    for w in range(4):                                       # 80 steps into 50 rows
        acts = torch.randint(0, 5, (T, N), dtype=torch.int64, device="cuda", generator=g)
        obs, rew, done = eng.rollout(acts)
        buf.add(prev, obs, rew, done, actions=acts)
        eng.sync()
        rr.store_window(ref, _host_bits(prev), _host_bits(obs), done.cpu().numpy(), [_host_bits(acts), _host_bits(rew), None], None, done_col=2)
        prev = obs[-1].clone()
    assert buf.size() == 50 and buf.pos == 30
    _same(buf.observations, ref.observations); _same(buf.next_observations, ref.next_observations)
    for name, exp in zip(buf.names, ref.columns):
        _same(buf.column(name), exp, name)
    drawn = buf.sample(64)
    sd = buf.state_dict()
    assert sd["cursor"] == [80, 1]
    other = DeviceReplayBuffer(eng, 50 * N, seed=0)
    other.load_state_dict(sd)
    assert other.cursor() == (80, 1) and other.seed == 21
    for a, b in zip([buf.observations, buf.next_observations] + buf.storage.col_rings, [other.observations, other.next_observations] + other.storage.col_rings):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    s1, s2 = buf.sample(64, extras=True), other.sample(64, extras=True)
    eng.sync()
    assert torch.equal(s1[1]["indices"], s2[1]["indices"]) and torch.equal(s1[0].observations, s2[0].observations)
    assert not torch.equal(s1[0].observations, drawn.observations)
    with pytest.raises(ValueError):
        DeviceReplayBuffer(eng, 49 * N).load_state_dict(sd)
    eng.close()


def test_indices_outside_are_rejected_and_an_empty_buffer_draws_nothing():
    """size * N, -1 and an index past the live rows of a partly filled buffer: their rows keep the sentinel, the others are gathered,
    sync() raises PTG_E_INDEX once; a device draw from an empty buffer writes nothing and raises too"""
    import torch
    from rl_ptg_amd import _lib
    from rl_ptg_amd.engine import PtgError
    N, S, F, B = 65, 5, 35, 40
    eng = _engine(N)
    pair = _Pair(eng, S, F, 4, [8, 4], 1, np.random.default_rng(5))

    def sentinels():
        return (torch.full((B, F), -777.25, dtype=torch.float32, device="cuda"), torch.full((B, F), -777.25, dtype=torch.float32, device="cuda"),
                [torch.full((B,), -3.5, dtype=torch.float64, device="cuda"), torch.full((B,), -3.5, dtype=torch.float32, device="cuda")],
                torch.full((B,), -9, dtype=torch.int64, device="cuda"))

    def untouched(out, rows):
        return all(bool((x[rows] == v).all()) for x, v in ((out[0], -777.25), (out[1], -777.25), (out[2][0], -3.5), (out[2][1], -3.5), (out[3], -9)))

    out = sentinels()
    eng.replay_sample(pair.st, batch_size=B, seed=1, out=out)                 # empty buffer
    with pytest.raises(PtgError) as ei:
        eng.sync()
    assert ei.value.code == _lib.E_INDEX and "ptg_replay_sample" in str(ei.value)
    eng.sync()
    assert untouched(out, slice(None))
    assert pair.st.cursor.cpu().tolist() == [0, 1]
    pair.add(3)                                              # 3 of 5 rows live
    pair.check()
    rng = np.random.default_rng(6)
    idx = rng.integers(0, 3 * N, B)
    bad = {3: 3 * N, 17: -1, 30: 4 * N + 2, 39: 2 ** 40}
    for b, v in bad.items():
        idx[b] = v
    good = np.array([b for b in range(B) if b not in bad])
    out = sentinels()
    eng.replay_sample(pair.st, idx=torch.from_numpy(idx).cuda(), out=out)
    with pytest.raises(PtgError) as ei:
        eng.sync()
    assert ei.value.code == _lib.E_INDEX
    eng.sync()                                               # reported once
    assert untouched(out, list(bad))
    eo, en, ecols = pair.ref.get_flat(idx[good])
    g = torch.from_numpy(good).cuda()
    _same(out[0][g], eo); _same(out[1][g], en); _same(out[2][0][g], ecols[0]); _same(out[2][1][g], ecols[1])
    assert np.array_equal(out[3][g].cpu().numpy(), idx[good])
    pair.check_sample(idx[good], "the call after")
    eng.close()


def test_device_drawn_indices_equal_the_restatement_and_spread():
    """idx_out equals the restated draw for (seed, cursor[1], row); the rows are a gather at idx_out; successive draws differ; with
    size * N = 192 and B = 65 536 every index is in range and every cell count within 341 +- 111 (B / 192, 6 sigma of the binomial,
    sigma = sqrt(B * (1/192) * (191/192)) = 18.4: a correct generator fails with probability below 1e-6)"""
    N, S, F = 64, 5, 4
    eng = _engine(N)
    pair = _Pair(eng, S, F, 4, [4], 0, np.random.default_rng(7))
    pair.add(3)
    pair.check()
    seed = 0x1234567890ABCDEF
    draws = []
    for c, B in enumerate([17, 17, 65536, 1]):
        o, n, outs, io = eng.replay_sample(pair.st, batch_size=B, seed=seed, want_idx=True)
        eng.sync()
        got = io.cpu().numpy()
        exp = rr.draw(seed, c, B, 3 * N)
        assert np.array_equal(got, exp), f"draw {c}"
        eo, en, ecols = pair.ref.get_flat(got)
        _same(o, eo); _same(n, en); _same(outs[0], ecols[0])
        draws.append(got)
    assert pair.st.cursor.cpu().tolist() == [3, 4]
    assert not np.array_equal(draws[0], draws[1])
    big = draws[2]
    assert big.min() >= 0 and big.max() < 192
    counts = np.bincount(big, minlength=192)
    print("cell counts of 65 536 draws over 192 cells: min", counts.min(), "max", counts.max())
    assert np.abs(counts - 65536 / 192).max() <= 111, (counts.min(), counts.max())
    o2, _, _, io2 = eng.replay_sample(pair.st, batch_size=17, seed=seed + 1, want_idx=True)         # another seed, the next counter
    eng.sync()
    assert np.array_equal(io2.cpu().numpy(), rr.draw(seed + 1, 4, 17, 3 * N))
    eng.close()


@pytest.mark.parametrize("out_dtype", ["float32", "float64"])
def test_normalised_rewards_equal_vn_normalize_frozen(out_dtype):
    """normalize_reward = vn_normalize(training=False) of the raw gathered rewards, bit for bit, with the statistics as they stand
    when the sample runs: after they have moved, and again after they have moved further; NaN and +-Inf rewards included"""
    import torch
    from rl_ptg_amd import DeviceReplayBuffer
    N, T, B = 64, 30, 64 * 3
    eng = _engine(N, "sb3_flat", out_dtype)
    eng.vn_init(gamma=0.97, clip_reward=1.5)
    buf = DeviceReplayBuffer(eng, 25 * N)
    g = torch.Generator(device="cuda"); g.manual_seed(3)
    prev = _clone(eng, eng.reset())
    acts = torch.randint(0, 5, (T, N), dtype=torch.int64, device="cuda", generator=g)
    obs, rew, done = eng.rollout(acts)
    rew[3, :4] = torch.tensor([float("nan"), float("inf"), float("-inf"), -0.0], dtype=rew.dtype, device="cuda")
    buf.add(prev, obs[:25], rew[:25], done[:25], actions=acts[:25])
    idx = torch.randint(0, 25 * N, (B,), device="cuda", generator=g)
    idx[:4] = torch.arange(3 * N, 3 * N + 4, device="cuda")
    raw = buf.sample(idx=idx).rewards
    for k in range(2):
        eng.vn_normalize(torch.nan_to_num(rew, nan=0.0, posinf=1.0, neginf=-1.0) * (k + 1), done)          # the statistics move
        before = eng.vn_get()
        got = buf.sample(idx=idx, normalize_reward=True).rewards
        padded = torch.zeros((3, N), dtype=rew.dtype, device="cuda")
        padded.view(-1)[:B] = raw[:, 0]
        exp = eng.vn_normalize(padded, torch.zeros((3, N), dtype=torch.uint8, device="cuda"), training=False).view(-1)[:B]
        eng.sync()
        _same(got[:, 0], _host_bits(exp), f"round {k}")
        after = eng.vn_get()
        assert before[0] == after[0]                         # sampling does not touch the statistics
        assert not torch.equal(got[4:], raw[4:]) and bool(torch.isnan(got[0, 0])) and got[1, 0] == 1.5 and got[2, 0] == -1.5
    _same(buf.sample(idx=idx).rewards, _host_bits(raw))      # stored raw
    eng.close()


def _equal_state(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_equal_state(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return a == b


def test_captured_step_add_and_draw_replayed_three_times():
    """step + add + device-drawn sample captured once on a replay-proof engine, on a side stream, and replayed three times: cursor,
    rings and each replay's batch equal the restatement advanced in step; env state apart from the steps taken, the finished-episode
    ring and the vn statistics are not touched by add / sample (an engine stepped alone agrees)"""
    import torch
    from rl_ptg_amd import DeviceReplayBuffer
    N, B = 70, 33
    eng, twin = _engine(N, "sb3_flat"), _engine(N, "sb3_flat")
    for e in (eng, twin):
        e.vn_init()
        e.set_replay_proof(True)
    buf = DeviceReplayBuffer(eng, 4 * N, columns={"actions": torch.int32}, seed=5)
    ref = rr.ReplayBuffer(4 * N, N, 40, np.int32, [np.int32, np.int32, np.int32])
    g = torch.Generator(device="cuda"); g.manual_seed(4)
    acts = torch.randint(0, 5, (6, N), dtype=torch.int32, device="cuda", generator=g)
    prev = _clone(eng, eng.reset())
    twin.reset()
    act_buf = torch.zeros(N, dtype=torch.int32, device="cuda")
    obs, rew, done, fin = eng.alloc_obs(zero=True), torch.zeros(N, dtype=torch.float32, device="cuda"), torch.zeros(N, dtype=torch.uint8, device="cuda"), eng.alloc_obs(zero=True)
    out = (torch.zeros((B, 40), device="cuda"), torch.zeros((B, 40), device="cuda"),
           [torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda")],
           torch.zeros(B, dtype=torch.int64, device="cuda"))

    def one():
        eng.step(act_buf, obs, rew, done, final_obs=fin)
        buf.add(prev, obs, rew, done, final_obs=fin, actions=act_buf)
        eng.replay_sample(buf.storage, batch_size=B, seed=buf.seed, out=out)
        prev.copy_(obs)

    def expect(t, p_host):
        twin.step(acts[t])
        twin.sync()
        o, r, d, f = _host_bits(twin.obs), _host_bits(twin.rew), twin.done.cpu().numpy(), _host_bits(twin.final_obs)
        rr.store_window(ref, p_host, o[None], d[None], [_host_bits(acts[t])[None], r[None], None], f[None], done_col=2)
        return o

    act_buf.copy_(acts[0])
    p_host = _host_bits(prev)
    one()                                                    # eager once: code objects are loaded before the capture
    eng.sync()
    p_host = expect(0, p_host)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            one()
    torch.cuda.current_stream().wait_stream(side)
    assert buf.cursor() == (1, 1)                            # capturing enqueued nothing
    for k in (1, 2, 3):
        act_buf.copy_(acts[k])
        graph.replay()
        torch.cuda.synchronize()
        p_host = expect(k, p_host)
        assert buf.cursor() == (k + 1, k + 1)
        _same(buf.observations, ref.observations, f"replay {k}"); _same(buf.next_observations, ref.next_observations, f"replay {k}")
        for name, exp in zip(buf.names, ref.columns):
            _same(buf.column(name), exp, f"replay {k} {name}")
        idx = rr.draw(5, k, B, min(k + 1, 4) * N)
        assert np.array_equal(out[3].cpu().numpy(), idx), f"replay {k}"
        eo, en, ecols = ref.get_flat(idx)
        _same(out[0], eo); _same(out[1], en)
        for got, exp in zip(out[2], ecols):
            _same(got, exp, f"replay {k}")
    eng.note_replays(3 - 1)                                  # three replays; the capture call counted as one step on the host
    eng.sync()
    a, b = eng.state_dict(), twin.state_dict()
    assert _equal_state(a["fields"], b["fields"]) and _equal_state(a["vn"], b["vn"])
    assert len(eng.finished_episodes()[0]) == len(twin.finished_episodes()[0]) == 0
    eng.close(); twin.close()


def test_add_and_sample_do_not_synchronise_the_host():
    """A condition, not a timing (as tests/test_minibatch.py checks minibatch): the stream is busy with milliseconds of fused steps
    before the calls and still busy when they have returned"""
    import torch
    from rl_ptg_amd import DeviceReplayBuffer
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    n, T, calls = 65536, 250, 8
    spec, _ = synthetic_spec(scenario=2, operation="OP2", eps_len_d=32)          # 4 608-step episodes: no boundary inside
    eng = HipEngine(spec.consts, spec.tables, spec.markets, n, device=0, out_dtype="float32", obs_layout="sb3_flat")
    eng.set_episode_plan(spec.eps_ind, n, n)
    eng.set_noise_rng(5)
    prev = _clone(eng, eng.reset())
    buf = DeviceReplayBuffer(eng, 4 * n, columns={"actions": torch.int32})
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    acts = torch.randint(0, 5, (T, n), dtype=torch.int32, device="cuda", generator=g)
    obs, rew, done = eng.alloc_obs(T), torch.empty((T, n), dtype=torch.float32, device="cuda"), torch.empty((T, n), dtype=torch.uint8, device="cuda")
    eng.rollout(acts, obs, rew, done)                                        # warm: first-launch work is not part of the condition
    buf.add(prev, obs[:2], rew[:2], done[:2], actions=acts[:2])
    out = eng.replay_sample(buf.storage, batch_size=256, want_idx=True)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    assert stream.query() is True
    for _ in range(calls):
        eng.rollout(acts, obs, rew, done)
    busy_before = stream.query()
    buf.add(obs[1], obs[2:5], rew[2:5], done[2:5], actions=acts[2:5])
    eng.replay_sample(buf.storage, batch_size=256, out=out)
    busy_after = stream.query()
    assert busy_before is False, "the rollouts were over before the calls: the check would prove nothing"
    assert busy_after is False, "the stream was idle when add and sample had returned: a call waited for the device"
    eng.sync()
    assert buf.cursor() == (5, 2) and buf.size() == 4 and buf.pos == 1
    assert torch.equal(buf.observations[2], obs[1]) and torch.equal(buf.next_observations[0], obs[4])     # step 4 went to slot 4 % 4
    i = out[3]
    assert torch.equal(out[0], buf.observations.view(-1, 40)[i]) and torch.equal(out[2][0], buf.column("actions").view(-1)[i])
    eng.close()


def test_refused_arguments_enqueue_nothing_and_a_valid_call_follows():
    import torch
    from rl_ptg_amd import _lib
    from rl_ptg_amd.engine import PtgError
    from rl_ptg_amd.replay import ReplayStorage
    N, S, F, T, B = 64, 5, 40, 3, 20
    eng = _engine(N)
    rng = np.random.default_rng(8)
    pair = _Pair(eng, S, F, 4, [8, 4], 1, rng)
    pair.add(2)
    pair.check()
    st = pair.st
    x, fin, done_h, cols_h = pair.window(T)
    prev, obs, fo, done = _dev(pair.last), _dev(x), _dev(fin), _dev(done_h)
    col8 = _dev(cols_h[0])
    idx_h = rng.integers(0, 2 * N, B)
    idx = torch.from_numpy(idx_h).cuda()
    out = (torch.full((B, F), -777.25, device="cuda"), torch.full((B, F), -777.25, device="cuda"),
           [torch.full((B,), -3.5, dtype=torch.float64, device="cuda"), torch.full((B,), -3.5, device="cuda")], torch.full((B,), -9, dtype=torch.int64, device="cuda"))
    rings_before = [_host_bits(t) for t in (st.obs_ring, st.next_ring, *st.col_rings, st.cursor)]
    torch.cuda.synchronize()

    def nothing_happened():
        assert torch.cuda.current_stream().query() is True
        for t, b in zip((st.obs_ring, st.next_ring, *st.col_rings, st.cursor), rings_before):
            assert np.array_equal(_host_bits(t), b)
        assert bool((out[0] == -777.25).all()) and bool((out[1] == -777.25).all()) and bool((out[2][0] == -3.5).all()) and bool((out[3] == -9).all())
        pair.check_sample(idx_h, "the valid call after a refusal")

    add = lambda **kw: eng.replay_add(kw.pop("st", st), kw.pop("prev", prev), kw.pop("obs", obs), kw.pop("cols", [col8, None]), done=kw.pop("done", done),
                                      final_obs=kw.pop("fo", fo), done_col=kw.pop("done_col", 1))
    smp = lambda **kw: eng.replay_sample(kw.pop("st", st), idx=kw.pop("idx", idx), out=kw.pop("out", out), **kw)
    long_obs = _dev(_bits((S + 1, N, F), 4, rng))
    b = dict(obs_cpu=obs.cpu(), obs_d=obs.double(), prev_t=prev.t().contiguous().t(), fo_st=_rows_view(fin, "fm"), col_cpu=col8.cpu(), col_f=col8.float(),
             col_t=col8.t().contiguous().t(), done_i=done.int(), idx_i=idx.int(), idx_cpu=idx.cpu(), idx_2d=idx.view(4, 5), idx_st=torch.cat([idx, idx])[::2],
             out0_d=out[0].double(), out0_t=torch.empty((F, B), device="cuda").t(), outc_f=torch.empty(B, device="cuda"), cur_f=st.cursor.float(),
             ring_h=st.obs_ring.half(), ring_t=torch.zeros((S, F, N), device="cuda").transpose(1, 2), dcol=torch.zeros((S, N), dtype=torch.int32, device="cuda"),
             cur_cpu=st.cursor.cpu(), ring_n=torch.zeros((S, N + 1, F), device="cuda"))
    torch.cuda.synchronize()
    refused = [
        (ValueError, lambda: add(obs=long_obs, fo=None)),                                # T = S + 1
        (ValueError, lambda: add(obs=obs[:0], fo=None)),                                 # T = 0
        (ValueError, lambda: add(obs=obs[0])),                                           # not a window
        (ValueError, lambda: add(obs=obs[:, :N - 1])),
        (ValueError, lambda: add(obs=obs[:, :, :F - 1])),
        (ValueError, lambda: add(obs=b["obs_cpu"])),
        (TypeError, lambda: add(obs=b["obs_d"])),
        (ValueError, lambda: add(prev=b["prev_t"])),                                     # prev_obs with other strides
        (ValueError, lambda: add(prev=prev[:N - 1])),
        (ValueError, lambda: add(fo=b["fo_st"])),                                        # final_obs with other strides
        (ValueError, lambda: add(fo=fo[:T - 1])),
        (ValueError, lambda: add(cols=[col8])),                                          # one column for two rings
        (ValueError, lambda: add(cols=[col8[:T - 1], None])),
        (ValueError, lambda: add(cols=[b["col_t"], None])),                              # [T, N], not contiguous
        (ValueError, lambda: add(cols=[b["col_cpu"], None])),
        (TypeError, lambda: add(cols=[b["col_f"], None])),                               # not the ring's dtype
        (ValueError, lambda: add(cols=[None, None])),                                    # a missing column
        (ValueError, lambda: add(done=None)),                                            # final_obs and the done column need done
        (TypeError, lambda: add(done=b["done_i"])),
        (ValueError, lambda: add(done=done[:T - 1])),
        (ValueError, lambda: add(done_col=2)),
        (TypeError, lambda: add(done_col=0)),                                            # an 8-byte done column
        (TypeError, lambda: add(st=st._replace(col_rings=[st.col_rings[0], b["dcol"]]))),        # a 4-byte done ring that is not float32
        (TypeError, lambda: add(st=st._replace(cursor=b["cur_f"]))),
        (ValueError, lambda: add(st=st._replace(cursor=b["cur_cpu"]))),
        (TypeError, lambda: add(st=st._replace(obs_ring=b["ring_h"], next_ring=b["ring_h"]))),
        (ValueError, lambda: add(st=st._replace(obs_ring=b["ring_t"]))),                 # a ring that is not contiguous
        (ValueError, lambda: add(st=st._replace(obs_ring=b["ring_n"], next_ring=b["ring_n"]))),  # rings of another env count
        (ValueError, lambda: add(st=st._replace(col_rings=[st.col_rings[0][:S - 1], st.col_rings[1]]))),
        (ValueError, lambda: add(st=st._replace(col_rings=[st.col_rings[0]] * 9), cols=[col8] * 9, done_col=-1)),
        (TypeError, lambda: smp(idx=b["idx_i"])),
        (TypeError, lambda: smp(idx=idx_h)),
        (ValueError, lambda: smp(idx=b["idx_cpu"])),
        (ValueError, lambda: smp(idx=b["idx_2d"])),
        (ValueError, lambda: smp(idx=b["idx_st"])),
        (ValueError, lambda: smp(batch_size=B + 1)),
        (ValueError, lambda: smp(idx=None)),                                             # neither indices nor a batch size
        (ValueError, lambda: smp(idx=None, batch_size=0)),
        (ValueError, lambda: smp(out=(b["out0_d"], out[1], out[2], out[3]))),
        (ValueError, lambda: smp(out=(b["out0_t"], out[1], out[2], out[3]))),
        (ValueError, lambda: smp(out=(out[0][:B - 1], out[1], out[2], out[3]))),
        (ValueError, lambda: smp(out=(out[0], out[1], [b["outc_f"], out[2][1]], out[3]))),
        (ValueError, lambda: smp(out=(out[0], out[1], out[2][:1], out[3]))),
        (ValueError, lambda: smp(out=(None, None, [None, None], None))),                 # no output
        (ValueError, lambda: smp(norm_col=2)),
        (TypeError, lambda: smp(norm_col=0)),                                            # a float64 column on a float32 engine
        (PtgError, lambda: smp(norm_col=1)),                                             # before vn_init: the library's refusal
    ]
    for k, (exc, call) in enumerate(refused):
        with pytest.raises(exc):
            call()
        nothing_happened()
    # the C entry points themselves
    L, h, stream = eng._L, eng._h, eng._stream()
    vp = C.c_void_p
    arr = lambda *ptrs: (vp * len(ptrs))(*ptrs)

    def desc(**kw):
        d = eng._replay_desc(st, "test")
        for k, v in kw.items():
            if k in ("col_bytes", "col_ring"):
                getattr(d, k)[v[0]] = v[1]
            else:
                setattr(d, k, v)
        return d

    def raw_add(d=None, handle=h, p=prev.data_ptr(), o=obs.data_ptr(), s_t=N * F, s_n=F, s_f=1, f=fo.data_ptr(), dn=done.data_ptr(), dc=1, k=2,
                src=arr(col8.data_ptr(), None), T_=T):
        d = desc() if d is None else d
        return L.ptg_replay_add(handle, C.byref(d) if d != "null" else None, p, o, s_t, s_n, s_f, f, dn, dc, k, src, T_, stream)

    def raw_smp(d=None, handle=h, i=idx.data_ptr(), batch=B, o0=out[0].data_ptr(), o1=out[1].data_ptr(), dst=arr(out[2][0].data_ptr(), out[2][1].data_ptr()),
                nc=-1, io=out[3].data_ptr()):
        d = desc() if d is None else d
        return L.ptg_replay_sample(handle, C.byref(d) if d != "null" else None, i, batch, 0, o0, o1, dst, nc, io, stream)

    bad_desc = [dict(capacity=0), dict(capacity=-3), dict(obs_dim=0), dict(obs_dim=(1 << 20) + 1), dict(obs_bytes=2), dict(obs_bytes=16), dict(obs_ring=None),
                dict(next_ring=None), dict(cursor_dev=None), dict(n_cols=9), dict(n_cols=-1), dict(col_bytes=(0, 3)), dict(col_bytes=(0, 16)), dict(col_ring=(1, None))]
    bad_add = [dict(d="null"), dict(handle=None), dict(p=None), dict(o=None), dict(T_=0), dict(T_=-2), dict(T_=S + 1), dict(s_t=-1), dict(s_n=-1), dict(s_f=-1),
               dict(k=1), dict(k=3), dict(src=None), dict(src=arr(None, None)), dict(dc=2), dict(dc=-2), dict(dc=0), dict(dn=None), dict(dn=None, f=None),
               dict(d=desc(col_bytes=(1, 8)))] + [dict(d=desc(**kw)) for kw in bad_desc]
    bad_smp = [dict(d="null"), dict(handle=None), dict(batch=0), dict(batch=-1), dict(nc=2), dict(nc=-2), dict(nc=1), dict(nc=0),
               dict(o0=None, o1=None, dst=None, io=None), dict(o0=None, o1=None, dst=arr(None, None), io=None)] + [dict(d=desc(**kw)) for kw in bad_desc]
    for fn, name, bad in ((raw_add, b"ptg_replay_add", bad_add), (raw_smp, b"ptg_replay_sample", bad_smp)):
        for kw in bad:
            assert fn(**kw) == _lib.E_INVALID, (name, kw)
            if "handle" not in kw:
                assert name in L.ptg_last_error(h)
            nothing_happened()
    assert raw_smp() == 0 and raw_add() == 0                                             # the same calls with good arguments
    rr.store_window(pair.ref, pair.last, x, done_h, cols_h, fin, 1)
    pair.last, pair.added = x[-1], pair.added + T
    pair.check("after the raw add")
    eo, en, ecols = pair.ref.get_flat(idx_h)                 # rows 0, 1 were live before and are not rewritten by 3 steps into slots 2, 3, 4
    _same(out[0], eo); _same(out[1], en); _same(out[2][0], ecols[0]); _same(out[2][1], ecols[1])
    eng.close()
