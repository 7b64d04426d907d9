"""ptg_minibatch / HipEngine.minibatch / HipEngine.minibatches (include/ptg_env.h) -- one shuffled PPO / A2C minibatch gathered
from the [T, N] buffers of a rollout on the device -- against the NumPy restatement of SB3's swap_and_flatten / RolloutBuffer.get
(tests/minibatch_restatement.py, pinned by tests/test_minibatch_host.py).

Every comparison is exact byte equality.  That is derived, not measured: the kernel copies, no arithmetic touches the payload.
Payloads are random BITS (so NaNs with payloads, infinities, subnormals and both zeros occur) with the special values planted as
well, and they are compared through integer views, host and device side, so that every bit counts.  Synthetic buffers are made
with the engines' own alloc_obs(T), so their layout (F, strides, pitch) is a real engine's."""
import ctypes as C

import numpy as np
import pytest

import minibatch_restatement as mr

pytestmark = pytest.mark.gpu

TS = [1, 2, 7, 64, 65]
NS = [1, 63, 64, 65, 257]
BS = [1, 63, 64, 65, "TN"]                                                # "TN": a permutation of all T * N rows
LAYOUTS = [("split", "mod", 16), ("sb3_flat", "raw", 31), ("row", "mod", 35), ("sb3_flat", "mod", 40)]      # 64, 124, 140, 160-byte float32 rows
DTYPES = ["float32", "float64"]
IDX = ["int32", "int64"]
INT_OF = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}
SPECIAL32 = np.array([0x7FC00000, 0x7FC12345, 0xFFC00001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF], np.uint32)
SPECIAL64 = np.array([0x7FF8000000000000, 0x7FF8000000012345, 0xFFF8000000000001, 0x7FF0000000000000, 0xFFF0000000000000,
                      0x8000000000000000, 0x0000000000000001, 0x800FFFFFFFFFFFFF], np.uint64)       # NaNs with payloads, +-Inf, -0.0, subnormals

_specs = {}


def _engine(n, layout="row", raw_modified="mod", out_dtype="float32", **kw):
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    if raw_modified not in _specs:
        _specs[raw_modified] = synthetic_spec(scenario=1, operation="OP1", eps_len_d=1, train_steps=400000, raw_modified=raw_modified)[0]
    s = _specs[raw_modified]
    return HipEngine(s.consts, s.tables, s.markets, n, device=0, out_dtype=out_dtype, obs_layout=layout, **kw)


def _bits(shape, itemsize, rng):
    """random bytes as an integer array of `itemsize`-byte elements, the special float values planted at the front"""
    a = rng.integers(0, 256, size=tuple(shape) + (itemsize,), dtype=np.uint8).view(INT_OF[itemsize])[..., 0].copy()
    if itemsize in (4, 8):
        sp = (SPECIAL32 if itemsize == 4 else SPECIAL64).view(INT_OF[itemsize])
        flat = a.reshape(-1)
        k = min(len(sp), flat.size)
        flat[:k] = sp[:k]
        flat[flat.size - k:] = sp[:k]
    return a


def _fill_obs(eng, T, x_bits):
    """an observation buffer of the engine's layout holding the bits of x_bits [T, N, F]"""
    import torch
    obs = eng.alloc_obs(T)
    eng.rows(obs).view(torch.int32 if x_bits.itemsize == 4 else torch.int64).copy_(torch.from_numpy(x_bits).cuda())
    return obs


def _host_bits(t):
    """device tensor -> host integer array of the same element size"""
    import torch
    iv = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]
    return t.contiguous().view(iv).cpu().numpy()


def _same(got, exp, what=""):
    g = _host_bits(got)
    assert g.shape == exp.shape and g.itemsize == exp.itemsize, (what, g.shape, exp.shape, g.dtype, exp.dtype)
    np.testing.assert_array_equal(g, exp.view(g.dtype), err_msg=what)


def _indices(T, N, B, idx_dtype, rng):
    if B == "TN":
        return rng.permutation(T * N).astype(idx_dtype)
    return rng.integers(0, T * N, B).astype(idx_dtype)


def _edge_cases():
    """The thinned product: every (N, layout) pair gets one engine, whose dtype, two T, two B and index types rotate through their
    lists -- 5 x 4 engines x 2 calls"""
    cases = []
    for i, N in enumerate(NS):
        for k, (layout, rm, F) in enumerate(LAYOUTS):
            calls = [(TS[(i + k + 2 * j) % 5], BS[(2 * i + k + 3 * j) % 5], IDX[(i + k + j) % 2]) for j in range(2)]
            cases.append((N, layout, rm, F, DTYPES[(i + k // 2 + k) % 2], calls))
    return cases


def test_the_thinned_product_meets_every_value_twice():
    cases = _edge_cases()
    count = {}
    for N, layout, rm, F, dtype, calls in cases:
        for T, B, it in calls:
            for key in (("N", N), ("F", F), ("dtype", dtype), ("T", T), ("B", B), ("idx", it), ("F-dtype", F, dtype)):
                count[key] = count.get(key, 0) + 1
    want = [("N", n) for n in NS] + [("F", l[2]) for l in LAYOUTS] + [("dtype", d) for d in DTYPES] + [("T", t) for t in TS] + \
           [("B", b) for b in BS] + [("idx", i) for i in IDX] + [("F-dtype", l[2], d) for l in LAYOUTS for d in DTYPES]
    assert all(count.get(k, 0) >= 2 for k in want), {k: count.get(k, 0) for k in want}


@pytest.mark.parametrize("i", range(len(NS)), ids=[f"N{n}" for n in NS])
def test_edges_of_rows_waves_and_paths(i):
    """T, N, B at 1, around the wave (64) and the 16-row share of a wave, several workgroups; 64- and 160-byte float32 rows and all
    float64 rows take the 16-byte path, 124- and 140-byte rows the element-wide one; int32 and int64 indices; with two columns"""
    import torch
    for N, layout, rm, F, dtype, calls in _edge_cases():
        if N != NS[i]:
            continue
        eng = _engine(N, layout, rm, dtype)
        assert eng.obs_dim == F
        size = 4 if dtype == "float32" else 8
        for T, B, it in calls:
            rng = np.random.default_rng([T, N, F, size])
            x = _bits((T, N, F), size, rng)
            c4, c1 = _bits((T, N), 4, rng), _bits((T, N), 1, rng)
            idx = _indices(T, N, B, it, rng)
            obs = _fill_obs(eng, T, x)
            got, (g4, g1) = eng.minibatch(torch.from_numpy(idx).cuda(), obs, [torch.from_numpy(c4).cuda(), torch.from_numpy(c1).cuda()])
            eng.sync()
            what = f"T={T} N={N} B={B} F={F} {dtype} {it}"
            assert got.shape == (len(idx), F) and got.dtype == obs.dtype and got.is_contiguous()
            _same(got, mr.gather(x, idx), what)
            _same(g4, mr.gather(c4, idx), what + " column int32")
            _same(g1, mr.gather(c1, idx), what + " column uint8")
        eng.close()


@pytest.mark.parametrize("dtype,N,pitch", [("float32", 65, None), ("float32", 65, 68), ("float64", 65, 68), ("float64", 8192, "auto")])
def test_feature_major_buffers_with_and_without_a_pitch(dtype, N, pitch):
    """[T, F, N] planes back to back, n + 3 elements apart, and the "auto" pitch of a float64 power-of-two batch: the gathered rows
    are those gathered from the rows() view copied contiguous"""
    import torch
    T = 5
    eng = _engine(N, "feature", "mod", dtype, obs_pitch=pitch)
    assert eng.feature_major and eng.pitch == {None: N, 68: 68, "auto": N + 128}[pitch]
    size = 4 if dtype == "float32" else 8
    rng = np.random.default_rng([N, size])
    x = _bits((T, N, eng.obs_dim), size, rng)
    obs = _fill_obs(eng, T, x)
    assert obs.shape == (T, eng.obs_dim, N) and obs.stride(1) == eng.pitch
    rows = eng.rows(obs).contiguous()
    _same(rows, x)
    for it, B in (("int32", "TN"), ("int64", 100)):
        idx = _indices(T, N, B, it, rng)
        got, _ = eng.minibatch(torch.from_numpy(idx).cuda(), obs)
        eng.sync()
        _same(got, mr.gather(_host_bits(rows), idx), f"{dtype} N={N} pitch={pitch} {it}")
    eng.close()


def test_columns_of_every_element_size_and_count():
    """0, 1, 6 and 8 columns of 1-, 2-, 4- and 8-byte elements; observations only; columns only (T from the columns)"""
    import torch
    T, N = 7, 65
    eng = _engine(N, "sb3_flat", "mod", "float32")
    rng = np.random.default_rng(11)
    x = _bits((T, N, eng.obs_dim), 4, rng)
    obs = _fill_obs(eng, T, x)
    sizes = [1, 4, 8, 2, 4, 4, 8, 1]
    tdt = {1: torch.uint8, 2: torch.int16, 4: torch.float32, 8: torch.float64}
    host = [_bits((T, N), s, rng) for s in sizes]
    dev = [torch.from_numpy(h).cuda().view(tdt[h.itemsize]) for h in host]
    for B in (1, 100, "TN"):
        idx = _indices(T, N, B, "int64", rng)
        idx_d = torch.from_numpy(idx).cuda()
        for k in (0, 1, 6, 8):
            for with_obs in (True, False):
                if k == 0 and not with_obs:
                    continue
                got, outs = eng.minibatch(idx_d, obs if with_obs else None, dev[:k])
                eng.sync()
                assert len(outs) == k and (got is None) == (not with_obs)
                if with_obs:
                    _same(got, mr.gather(x, idx), f"obs with {k} columns")
                for c in range(k):
                    assert outs[c].dtype == dev[c].dtype and outs[c].shape == (len(idx),)
                    _same(outs[c], mr.gather(host[c], idx), f"column {c} of {k}, {sizes[c]} bytes, obs={with_obs}")
    eng.close()


def test_permutation_slices_arange_and_repeats():
    """All slices of one randperm(T * N), batch size not dividing it: the outputs concatenated are a permutation of the source rows,
    every row once.  arange is the [N, T] transposition.  Repeated indices, and one index B times, are legal."""
    import torch
    T, N, bs = 21, 13, 50                                    # 273 rows: five batches of 50 and one of 23
    eng = _engine(N, "row", "mod", "float32")
    F = eng.obs_dim
    tag = (np.arange(T)[:, None] * 1000 + np.arange(N)[None, :]).astype(np.int32)       # tag[t, n] names (t, n)
    x = (tag[:, :, None] * 64 + np.arange(F, dtype=np.int32)[None, None, :]).astype(np.int32)
    obs = _fill_obs(eng, T, x)
    col = torch.from_numpy(tag).cuda()
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    perm = torch.randperm(T * N, device="cuda", generator=g)
    batches = list(eng.minibatches(perm, bs, obs, [col]))
    eng.sync()
    assert [b[0].shape[0] for b in batches] == [50] * 5 + [23]
    assert len({b[0].data_ptr() for b in batches}) == len(batches)          # fresh outputs per yield
    rows, tags = torch.cat([b[0] for b in batches]), torch.cat([b[1][0] for b in batches])
    p = perm.cpu().numpy()
    _same(rows, mr.gather(x, p)); _same(tags, mr.gather(tag, p))
    assert np.array_equal(np.sort(_host_bits(tags)), np.sort(tag.reshape(-1)))          # every (t, n) exactly once
    ref = list(mr.minibatches(p, bs, x, [tag]))
    for (o, (c,)), (eo, (ec,)) in zip(batches, ref):
        _same(o, eo); _same(c, ec)
    (one_o, (one_c,)), = list(eng.minibatches(perm, None, obs, [col]))                  # A2C: batch_size None
    got, (gc,) = eng.minibatch(torch.arange(T * N, device="cuda"), obs, [col])
    rep = np.array([5, 5, 272, 0, 5, 272, 0, 0, 131] * 9, np.int32)
    got_r, (gc_r,) = eng.minibatch(torch.from_numpy(rep).cuda(), obs, [col])
    same = np.full(77, 131, np.int64)
    got_s, (gc_s,) = eng.minibatch(torch.from_numpy(same).cuda(), obs, [col])
    eng.sync()
    _same(one_o, mr.gather(x, p)); _same(one_c, mr.gather(tag, p))
    _same(got.view(N, T, F), np.ascontiguousarray(x.transpose(1, 0, 2))); _same(gc.view(N, T), np.ascontiguousarray(tag.T))
    _same(got_r, mr.gather(x, rep)); _same(gc_r, mr.gather(tag, rep))
    _same(got_s, mr.gather(x, same)); _same(gc_s, mr.gather(tag, same))
    eng.close()


def test_behind_the_real_pipeline():
    """rollout -> vn_normalize -> gae -> minibatches on an sb3_flat engine, 20 steps, PPO's batch size 203 (not dividing 20 * 70):
    every batch is the restatement's on the host copies of the same tensors"""
    import torch
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    n, T = 70, 20
    spec, _ = synthetic_spec(scenario=2, operation="OP2", eps_len_d=1, train_steps=200000)
    eng = HipEngine(spec.consts, spec.tables, spec.markets, n, device=0, out_dtype="float32", obs_layout="sb3_flat")
    eng.set_episode_plan(spec.eps_ind, n, n)
    eng.set_noise_rng(seed=3)
    eng.vn_init(gamma=0.973)
    eng.reset()
    g = torch.Generator(device="cuda"); g.manual_seed(8)
    acts = torch.randint(0, 5, (T, n), dtype=torch.int64, device="cuda", generator=g)
    values = torch.randn((T, n), dtype=torch.float32, device="cuda", generator=g)
    logp = torch.randn((T, n), dtype=torch.float32, device="cuda", generator=g)
    last_values = torch.randn((n,), dtype=torch.float32, device="cuda", generator=g)
    obs, rew, done = eng.rollout(acts)
    adv, ret = eng.gae(eng.vn_normalize(rew, done), values, done, last_values, 0.973, 0.8002)
    cols = [acts, values, logp, adv, ret, done]
    perm = torch.randperm(T * n, device="cuda", generator=g)
    batches = list(eng.minibatches(perm, 203, obs, cols))
    eng.sync()
    assert obs.shape == (T, n, 40) and [b[0].shape[0] for b in batches] == [203] * 6 + [T * n - 6 * 203]
    ref = list(mr.minibatches(perm.cpu().numpy(), 203, _host_bits(obs), [_host_bits(c) for c in cols]))
    assert len(ref) == len(batches)
    for k, ((o, cs), (eo, ecs)) in enumerate(zip(batches, ref)):
        _same(o, eo, f"batch {k} observations")
        for c, (got, exp) in enumerate(zip(cs, ecs)):
            assert got.dtype == cols[c].dtype
            _same(got, exp, f"batch {k} column {c}")
    eng.close()


def test_byte_offsets_past_4_gib():
    """float32 [410, 65 536, 40] is 4 299 161 600 bytes, the first T past 2^32 at this width.  Element i holds int32(i) (i < 2^31), so
    the expected rows are a closed form; 257 rows: the first, the last, the one across the 2^32-byte boundary and its neighbours."""
    import torch
    T, N, F = 410, 65536, 40
    free = torch.cuda.mem_get_info()[0]
    if free < 6 * 2 ** 30:
        print(f"test_byte_offsets_past_4_gib skipped: {free / 2 ** 30:.2f} GiB of device memory free, 6 GiB needed")
        pytest.skip(f"{free / 2 ** 30:.2f} GiB of device memory free, 6 GiB needed")
    eng = _engine(N, "sb3_flat", "mod", "float32")
    assert eng.obs_dim == F and T * N * F * 4 > 2 ** 32 > (T - 1) * N * F * 4 and T * N * F < 2 ** 31
    obs = eng.alloc_obs(T)
    flat = obs.view(torch.int32).view(-1)
    step = 16 * N * F
    for a in range(0, T * N * F, step):
        b = min(a + step, T * N * F)
        flat[a:b].copy_(torch.arange(a, b, dtype=torch.int32, device="cuda"))
    r0 = 2 ** 32 // (F * 4)                                  # the source row [t, n] -> t * N + n that holds byte 2^32
    assert r0 * F * 4 < 2 ** 32 < (r0 + 1) * F * 4
    src_rows = np.array([0, T * N - 1, r0 - 1, r0, r0 + 1, r0 - N, r0 + 2], np.int64)
    rng = np.random.default_rng(9)
    src_rows = np.concatenate([src_rows, rng.integers(0, T * N, 257 - len(src_rows))])
    t, n = src_rows // N, src_rows % N
    idx = n * T + t                                          # SB3's flat order
    rng.shuffle(idx)
    t, n = idx % T, idx // T
    expect = ((t * N + n)[:, None] * F + np.arange(F)[None, :]).astype(np.int32)
    col = torch.arange(T * N, dtype=torch.int32, device="cuda").view(T, N)
    for it in ("int64", "int32"):
        got, (gc,) = eng.minibatch(torch.from_numpy(idx.astype(it)).cuda(), obs, [col])
        eng.sync()
        _same(got, expect, it)
        _same(gc, (t * N + n).astype(np.int32), it)
    del obs, flat
    eng.close()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("it", IDX)
@pytest.mark.parametrize("layout,F", [("sb3_flat", 40), ("row", 35)])
def test_indices_just_outside_are_rejected(it, layout, F):
    """T * N and -1 among valid indices: their rows and column entries keep the sentinel, the valid ones are gathered, sync() raises
    PTG_E_INDEX once, and the next call is fine"""
    import torch
    from rl_ptg_amd import _lib
    from rl_ptg_amd.engine import PtgError
    T, N, B = 7, 65, 40
    eng = _engine(N, layout, "mod", "float32")
    rng = np.random.default_rng(12)
    x, c = _bits((T, N, F), 4, rng), _bits((T, N), 8, rng)
    obs, col = _fill_obs(eng, T, x), torch.from_numpy(c).cuda()
    idx = rng.integers(0, T * N, B).astype(it)
    bad = {3: T * N, 17: -1}
    for b, v in bad.items():
        idx[b] = v
    good = np.array([b for b in range(B) if b not in bad])
    out = torch.full((B, F), -777.25, dtype=torch.float32, device="cuda")
    out_c = torch.full((B,), -12345, dtype=torch.int64, device="cuda")
    eng.minibatch(torch.from_numpy(idx).cuda(), obs, [col], obs_out=out, columns_out=[out_c])
    with pytest.raises(PtgError) as ei:
        eng.sync()
    assert ei.value.code == _lib.E_INDEX == -5 and "ptg_minibatch" in str(ei.value)
    eng.sync()                                               # reported once
    o, oc = out.cpu().numpy(), out_c.cpu().numpy()
    assert np.array_equal(o[good].view(np.int32), mr.gather(x, idx[good]))
    assert np.array_equal(oc[good], mr.gather(c, idx[good]))
    assert (o[list(bad)] == -777.25).all() and (oc[list(bad)] == -12345).all()
    got, (gc,) = eng.minibatch(torch.from_numpy(idx[good]).cuda(), obs, [col])
    eng.sync()
    _same(got, mr.gather(x, idx[good])); _same(gc, mr.gather(c, idx[good]))
    eng.close()


def _rolled_engine(n, T, seed):
    """an sb3_flat engine behind a T-step rollout with reward normalisation: state, finished-episode ring and vn statistics are live"""
    import torch
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    spec, _ = synthetic_spec(scenario=2, operation="OP2", eps_len_d=1, train_steps=200000)      # 139-step episodes
    eng = HipEngine(spec.consts, spec.tables, spec.markets, n, device=0, out_dtype="float32", obs_layout="sb3_flat")
    eng.set_episode_plan(spec.eps_ind, n, n)
    eng.set_noise_rng(seed=seed)
    eng.vn_init()
    eng.reset()
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    acts = torch.randint(0, 5, (T, n), dtype=torch.int32, device="cuda", generator=g)
    obs, rew, done = eng.rollout(acts)
    rew_n = eng.vn_normalize(rew, done)
    eng.sync()
    return eng, obs, [acts, rew_n, done], g


def _equal_state(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_equal_state(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return a == b


def test_side_stream_capture_replay_and_untouched_state():
    """On a side stream; captured once into a graph and replayed three times with other contents in the static idx tensor, each replay
    giving that replay's minibatch; env state, normaliser and the finished-episode ring as they were"""
    import torch
    n, T, B = 100, 150, 203                                  # crosses the episode end at step 139: n finished episodes in the ring
    eng, obs, cols, g = _rolled_engine(n, T, 31)
    assert int(cols[2].sum()) == n
    before = eng.state_dict()
    x, hc = _host_bits(obs), [_host_bits(c) for c in cols]
    perm = torch.randperm(T * n, device="cuda", generator=g)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got, outs = eng.minibatch(perm[:B], obs, cols)
    side.synchronize()
    p = perm.cpu().numpy()
    _same(got, mr.gather(x, p[:B]))
    for o, h in zip(outs, hc):
        _same(o, mr.gather(h, p[:B]))
    idx_static = perm[:B].clone()
    out = torch.zeros((B, obs.shape[2]), dtype=obs.dtype, device="cuda")
    outs = [torch.zeros((B,), dtype=c.dtype, device="cuda") for c in cols]
    graph = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            eng.minibatch(idx_static, obs, cols, obs_out=out, columns_out=outs)
    torch.cuda.current_stream().wait_stream(side)
    for k in (1, 2, 3):
        idx_static.copy_(perm[k * B:(k + 1) * B])
        graph.replay()
        torch.cuda.synchronize()
        _same(out, mr.gather(x, p[k * B:(k + 1) * B]), f"replay {k}")
        for o, h in zip(outs, hc):
            _same(o, mr.gather(h, p[k * B:(k + 1) * B]), f"replay {k}")
    eng.sync()
    assert _equal_state(before, eng.state_dict())
    assert len(eng.finished_episodes()[0]) == n              # the ring still holds the rollout's finished episodes
    eng.close()


def test_minibatch_does_not_synchronise_the_host():
    """A condition, not a timing (as tests/test_gae.py checks gae): 2 000 fused steps at 65 536 envs are milliseconds of device time,
    far more than the host needs to enqueue them and the call behind them.  The stream is busy before the call and still busy when
    it has returned."""
    import torch
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    n, T, calls, B = 65536, 250, 8, 203
    spec, _ = synthetic_spec(scenario=2, operation="OP2", eps_len_d=32)          # 4 608-step episodes: no boundary inside
    eng = HipEngine(spec.consts, spec.tables, spec.markets, n, device=0, out_dtype="float32", obs_layout="sb3_flat")
    eng.set_episode_plan(spec.eps_ind, n, n)
    eng.set_noise_rng(5)
    eng.reset()
    assert eng.steps_to_episode_end() > T * (calls + 1)
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    acts = torch.randint(0, 5, (T, n), dtype=torch.int32, device="cuda", generator=g)
    obs = eng.alloc_obs(T)
    rew = torch.empty((T, n), dtype=torch.float32, device="cuda")
    done = torch.empty((T, n), dtype=torch.uint8, device="cuda")
    idx = torch.randint(0, T * n, (B,), dtype=torch.int64, device="cuda", generator=g)
    out = torch.empty((B, eng.obs_dim), dtype=torch.float32, device="cuda")
    outs = [torch.empty((B,), dtype=torch.float32, device="cuda"), torch.empty((B,), dtype=torch.uint8, device="cuda")]
    eng.rollout(acts, obs, rew, done)                                        # warm: first-launch work is not part of the condition
    eng.minibatch(idx, obs, [rew, done], obs_out=out, columns_out=outs)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    assert stream.query() is True
    for _ in range(calls):
        eng.rollout(acts, obs, rew, done)
    busy_before = stream.query()
    eng.minibatch(idx, obs, [rew, done], obs_out=out, columns_out=outs)
    busy_after = stream.query()
    assert busy_before is False, "the rollouts were over before minibatch was called: the check would prove nothing"
    assert busy_after is False, "the stream was idle when minibatch returned: the call waited for the device"
    eng.sync()
    t, e = idx % T, idx // T                                                 # 203 rows of the 2.6 GB buffer, picked on the device
    _same(out, _host_bits(obs[t, e])); _same(outs[0], _host_bits(rew[t, e])); _same(outs[1], _host_bits(done[t, e]))
    eng.close()


def test_refused_arguments_enqueue_nothing_and_a_valid_call_follows():
    import torch
    from rl_ptg_amd import _lib
    from rl_ptg_amd.engine import PtgError
    T, N, B = 6, 64, 50
    eng = _engine(N, "sb3_flat", "mod", "float32")
    F = eng.obs_dim
    rng = np.random.default_rng(13)
    x, c = _bits((T, N, F), 4, rng), _bits((T, N), 4, rng)
    obs, col = _fill_obs(eng, T, x), torch.from_numpy(c).cuda()
    idx_h = rng.integers(0, T * N, B)
    idx = torch.from_numpy(idx_h).cuda()
    out = torch.full((B, F), -777.25, dtype=torch.float32, device="cuda")
    out_c = torch.full((B,), -12345, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def valid():
        """nothing was enqueued by the refused call before; the same buffers are fine with good arguments"""
        assert torch.cuda.current_stream().query() is True
        assert bool((out == -777.25).all()) and bool((out_c == -12345).all())
        got, (gc,) = eng.minibatch(idx, obs, [col])
        eng.sync()
        _same(got, mr.gather(x, idx_h)); _same(gc, mr.gather(c, idx_h))

    m = lambda *a, **kw: eng.minibatch(*a, obs_out=kw.pop("obs_out", out), columns_out=kw.pop("columns_out", [out_c]), **kw)
    # every argument a refusal needs is made BEFORE the calls, so that the stream is idle around each of them
    b = dict(idx_f=idx.float(), idx_16=idx.to(torch.int16), idx_2d=idx.view(5, 10), idx_st=torch.cat([idx, idx])[::2], idx_cpu=idx.cpu(),
             obs_cpu=obs.cpu(), col_cpu=col.cpu(), out_cpu=out.cpu(), outc_cpu=out_c.cpu(), col_nt=col.t().contiguous(),
             col_st=col.t().contiguous().t(), col_c128=col.to(torch.complex128), obs_st=obs.transpose(1, 2).contiguous().transpose(1, 2),
             obs_h=obs.half(), out_d=out.double(), out_t=torch.empty((F, B), device="cuda").t(), outc_f=out_c.float())
    torch.cuda.synchronize()
    refused = [
        (TypeError, lambda: m(b["idx_f"], obs, [col])),
        (TypeError, lambda: m(b["idx_16"], obs, [col])),
        (TypeError, lambda: m(idx_h, obs, [col])),                                       # a host array
        (ValueError, lambda: m(b["idx_2d"], obs, [col])),
        (ValueError, lambda: m(b["idx_st"], obs, [col])),                                # 1-D, strided
        (ValueError, lambda: m(b["idx_cpu"], obs, [col])),                               # wrong device
        (ValueError, lambda: m(idx, b["obs_cpu"], [col])),
        (ValueError, lambda: m(idx, obs, [b["col_cpu"]])),
        (ValueError, lambda: m(idx, obs, [col], obs_out=b["out_cpu"])),
        (ValueError, lambda: m(idx, obs, [col], columns_out=[b["outc_cpu"]])),
        (ValueError, lambda: m(idx, obs, [col[:T - 1]])),                                # columns that are not [T, N]
        (ValueError, lambda: m(idx, obs, [col[:, :N - 1]])),
        (ValueError, lambda: m(idx, obs, [col.t()])),
        (ValueError, lambda: m(idx, obs, [col.view(-1)])),
        (ValueError, lambda: m(idx, obs, [b["col_st"]])),                                # [T, N], not contiguous
        (ValueError, lambda: m(idx, None, [b["col_nt"]], obs_out=None)),                 # columns only: T from the column, N wrong
        (TypeError, lambda: m(idx, obs, [b["col_c128"]])),                               # 16-byte elements
        (ValueError, lambda: m(idx, obs[:, :, :F - 1], [col])),                          # not a buffer of alloc_obs
        (ValueError, lambda: m(idx, obs[:, :N - 1], [col])),
        (ValueError, lambda: m(idx, obs[0], [col])),
        (ValueError, lambda: m(idx, b["obs_st"], [col])),                                # the shape, other strides
        (TypeError, lambda: m(idx, b["obs_h"], [col])),
        (ValueError, lambda: m(idx, obs, [col], obs_out=out[:B - 1])),                   # mismatched outputs
        (ValueError, lambda: m(idx, obs, [col], obs_out=b["out_d"])),
        (ValueError, lambda: m(idx, obs, [col], obs_out=b["out_t"])),
        (ValueError, lambda: m(idx, obs, [col], columns_out=[out_c[:B - 1]])),
        (ValueError, lambda: m(idx, obs, [col], columns_out=[b["outc_f"]])),
        (ValueError, lambda: m(idx, obs, [col], columns_out=[])),
        (ValueError, lambda: m(idx, obs, [col], columns_out=[out_c, out_c])),
        (ValueError, lambda: m(idx, None, [col])),                                       # an output for observations that are not given
        (ValueError, lambda: m(idx, obs, [col] * 9, columns_out=[out_c] * 9)),           # more than 8 columns
        (ValueError, lambda: m(idx, None, [], obs_out=None, columns_out=None)),          # nothing to gather
        (PtgError, lambda: m(idx[:0], obs, [col], obs_out=out[:0], columns_out=[out_c[:0]])),      # B = 0: the library's refusal
        (PtgError, lambda: m(idx, obs[:0], [col[:0]])),                                  # T = 0
    ]
    for k, (exc, call) in enumerate(refused):
        with pytest.raises(exc):
            call()
        valid()
    # the C entry point itself
    L, h, st = eng._L, eng._h, eng._stream()
    vp = C.c_void_p
    arr = lambda *ptrs: (vp * len(ptrs))(*ptrs)

    def raw(handle=h, i=idx.data_ptr(), ib=8, batch=B, T_=T, o=obs.data_ptr(), ob=4, dim=F, oo=out.data_ptr(), k=1, src=arr(col.data_ptr()),
            sz=(C.c_int32 * 1)(4), dst=arr(out_c.data_ptr()), s_t=N * F):
        return L.ptg_minibatch(handle, vp(i) if i else None, ib, batch, T_, vp(o) if o else None, s_t, F, 1, dim, ob, vp(oo) if oo else None,
                               k, src, sz, dst, st)

    nine = arr(*[col.data_ptr()] * 9)
    bad = [dict(handle=None), dict(i=None), dict(ib=2), dict(ib=0), dict(batch=0), dict(batch=-4), dict(T_=0), dict(T_=-1), dict(ob=2), dict(ob=16),
           dict(dim=0), dict(s_t=-1), dict(o=None), dict(oo=None), dict(k=9, src=nine, sz=(C.c_int32 * 9)(*[4] * 9), dst=nine), dict(k=-1),
           dict(src=None), dict(sz=None), dict(dst=None), dict(src=arr(None)), dict(dst=arr(None)), dict(sz=(C.c_int32 * 1)(3)),
           dict(sz=(C.c_int32 * 1)(16)), dict(sz=(C.c_int32 * 1)(0)), dict(o=None, oo=None, k=0)]
    for kw in bad:
        assert raw(**kw) == _lib.E_INVALID, kw
        if "handle" not in kw:
            assert b"ptg_minibatch" in L.ptg_last_error(h)
            with pytest.raises(PtgError):
                eng._chk(raw(**kw))
        valid()
    assert raw() == 0                                                                    # the same call with good arguments
    eng.sync()
    _same(out, mr.gather(x, idx_h)); _same(out_c, mr.gather(c, idx_h))
    eng.close()
