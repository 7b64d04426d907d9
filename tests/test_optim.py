"""ptg_optim_step, HipEngine.optim_plan / optim_step / polyak_update and rl_ptg_amd.DeviceOptimizer (include/ptg_env.h) -- grad-norm clip,
Adam / RMSprop, Polyak and zero_grad for all tensors of an optimiser in at most three launches -- against the NumPy restatement
(tests/optim_restatement.py, pinned against torch.optim by tests/test_optim_host.py).

Bounds, derived and not measured.  The kernels compute every element in float64 with correctly rounded +, *, / and sqrt and round once
on the store, and so does the restatement: parameters, both state tensors and targets are compared BIT FOR BIT through integer views,
the restatement being fed the kernel's own total norm -- the one quantity that depends on a summation order.  That norm is compared
separately with sqrt(math.fsum(g * g)): a partial sum of non-negative terms passes through at most d = 22 + ceil(n_chunks / 256)
roundings on the device (the header counts them), the square root halves the relative error and adds one rounding, and the reference
itself is within 1.5 * 2^-53 -- together below the (d + 2) * 2^-53 relative bound asserted here."""
import ctypes as C
import math

import numpy as np
import pytest

import optim_restatement as orr

pytestmark = pytest.mark.gpu

SENTINEL = 7.5
LR, EPS, ALPHA, BETAS, TAU = 1e-2, 1e-5, 0.99, (0.9, 0.999), 0.005
DTYPES = [np.float32, np.float64]
_engines = {}
_spec = []


def _engine(n=64, fresh=False):
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    if not fresh and n in _engines:
        return _engines[n]
    if not _spec:
        _spec.append(synthetic_spec(scenario=2, operation="OP2", eps_len_d=1, train_steps=200000)[0])
    s = _spec[0]
    eng = HipEngine(s.consts, s.tables, s.markets, n, device=0, out_dtype="float32", obs_layout="sb3_flat")
    eng.set_episode_plan(s.eps_ind, n, n)
    eng.set_noise_rng(seed=4)
    if not fresh:
        _engines[n] = eng
    return eng


def _chunk():
    return _engine().optim_chunk()


def _numels():
    """the smallest sizes at which the kernels can go wrong: one element, below / at / above a wave, below / at / above a chunk, two
    chunks and a ragged third"""
    c = _chunk()
    return [1, 3, 63, 64, 65, c - 1, c, c + 1, 2 * c + 7]


def _lists():
    """lists of 1, 2 and 13 tensors mixing the sizes"""
    ns = _numels()
    return [[ns[-1]], [ns[4], ns[6]], ns + [2, ns[5], 66, ns[7]]]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(got, want, nan_ok=False):
    """bit equality; nan_ok: a NaN must meet a NaN (payload and sign of a NaN are not part of the contract), everything else bit for bit"""
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if not nan_ok:
        return bool(np.array_equal(_bits(got), _bits(want)))
    n = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), n) and np.array_equal(_bits(got)[~n], _bits(want)[~n]))


def _allocations():
    """how many device allocations the caching allocator has served so far"""
    import torch
    return torch.cuda.memory_stats()["allocation.all.allocated"]


def _equal_state(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_equal_state(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return a == b


class Flat:
    """tensors as views into ONE flat buffer with guard elements (SENTINEL) before, between and after them.  odd: every view starts at
    an odd element offset (8-byte aligned at most: the element-wise path); else at a multiple of four elements (16-byte aligned)"""

    def __init__(self, numels, dt, odd, fill):
        self.numels, self.dt = list(numels), dt
        self.starts, pos = [], 4
        for n in self.numels:
            start = (pos + 3) // 4 * 4 + (1 if odd else 0)
            self.starts.append(start)
            pos = start + n + 3
        self.host = np.full((pos + 3) // 4 * 4 + 4, SENTINEL, dtype=dt)
        for k, a in enumerate(fill):
            self.views(self.host)[k][:] = a
        self.dev = None

    def views(self, flat):
        return [flat[s:s + n] for s, n in zip(self.starts, self.numels)]

    def upload(self):
        import torch
        self.dev = torch.from_numpy(self.host.copy()).cuda()
        v = self.views(self.dev)
        for x in v:
            assert x.is_contiguous() and (x.data_ptr() % 16 == 0) == (self.starts[0] % 4 == 0)
        return v

    def expect(self, arrays):
        """the flat buffer with the views replaced: what the device buffer must equal, guards included"""
        out = self.host.copy()
        for k, a in enumerate(arrays):
            self.views(out)[k][:] = a
        return out


def _data(numels, dt, seed):
    rng = np.random.default_rng(seed)
    return [rng.normal(size=n).astype(dt) for n in numels]


def _depth(n_chunks):
    return 22 + (n_chunks + 255) // 256


def _check_norm(total, grads, n_chunks):
    ref = orr.total_norm(grads)
    bound = (_depth(n_chunks) + 2) * 2.0 ** -53 * ref
    assert abs(total - ref) <= bound, (total, ref, bound)
    return abs(total - ref) / bound if bound else 0.0


class Run:
    """one optimiser on the device and its restatement side by side"""

    def __init__(self, eng, numels, dt, kind, odd, targets, seed=0, p_data=None):
        self.eng, self.kind, self.dt, self.numels = eng, kind, dt, numels
        self.fp, self.fg = Flat(numels, dt, odd, p_data or _data(numels, dt, seed)), Flat(numels, dt, odd, _data(numels, dt, seed + 1))
        self.fq = Flat(numels, dt, odd, _data(numels, dt, seed + 2)) if targets else None
        self.params, self.grads = self.fp.upload(), self.fg.upload()
        self.targets = self.fq.upload() if targets else None
        self.plan = eng.optim_plan(self.params, self.grads, kind, targets=self.targets)
        self.h_p, self.h_g = self.fp.views(self.fp.host.copy()), self.fg.views(self.fg.host.copy())
        self.h_q = self.fq.views(self.fq.host.copy()) if targets else None
        self.h_s1, self.h_s2 = [np.zeros(n, dt) for n in numels], [np.zeros(n, dt) for n in numels]
        self.st = orr.new_state()
        self.norm_err = 0.0

    def set_grads(self, arrays):
        import torch
        self.h_g = [np.asarray(a, self.dt).copy() for a in arrays]
        for v, a in zip(self.grads, self.h_g):
            v.copy_(torch.from_numpy(a))
        self.fg.host = self.fg.expect(self.h_g)

    def device_step(self, lr=LR, max_norm=None, zero_grad=False):
        self.eng.optim_step(self.plan, lr, betas=BETAS, eps=EPS, alpha=ALPHA, max_grad_norm=max_norm, tau=TAU if self.targets else None, zero_grad=zero_grad)

    def check(self, lr=LR, max_norm=None, zero_grad=False, nan_ok=False, sync=True):
        """after a device step: read back the total norm, take the restatement's step with it, compare every buffer"""
        import torch
        if sync:
            self.eng.sync()
        else:
            torch.cuda.synchronize()
        total = None
        if max_norm is not None:
            total = float(self.plan.norm[0])
            if not nan_ok:
                self.norm_err = max(self.norm_err, _check_norm(total, self.h_g, self.plan.n_chunks))
        r = orr.step(self.kind, self.h_p, self.h_g, self.h_s1, self.h_s2, self.st, lr, betas=BETAS, eps=EPS, alpha=ALPHA, max_norm=max_norm,
                     targets=self.h_q, tau=TAU if self.targets else None, total=total, zero_grad=zero_grad)
        self.h_p, self.h_s1, self.h_g = r["params"], r["state1"], r["grads"]
        if self.kind == "adam":
            self.h_s2 = r["state2"]
        assert _same(self.fp.dev.cpu().numpy(), self.fp.expect(self.h_p), nan_ok), "parameters (or their guards)"
        assert _same(self.fg.dev.cpu().numpy(), self.fg.expect(self.h_g), nan_ok), "gradients (or their guards)"
        for k in range(len(self.numels)):
            assert _same(self.plan.state1[k].cpu().numpy(), self.h_s1[k], nan_ok), ("state 1", k)
            if self.kind == "adam":
                assert _same(self.plan.state2[k].cpu().numpy(), self.h_s2[k], nan_ok), ("state 2", k)
        if self.targets:
            self.h_q = r["targets"]
            assert _same(self.fq.dev.cpu().numpy(), self.fq.expect(self.h_q), nan_ok), "targets (or their guards)"
        dev_state = self.plan.state.cpu().numpy()
        want = [self.st["t"], self.st["p1"], self.st["p2"]] if self.kind == "adam" else [self.st["t"], 1.0, 1.0]
        assert dev_state[:3].tolist() == want, (dev_state, want)
        return r


@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_every_shape_path_and_flag_bit_for_bit(dt, kind):
    """lists of 1, 2 and 13 tensors x views at odd element offsets (element-wise) and 16-byte aligned (vector path) x clip active
    (total > max_norm) / inactive (coefficient exactly 1.0) / None x with and without targets x with and without the zero-grad flag;
    three consecutive steps each (the bias correction), fresh gradients before each; guards between the views keep their bits"""
    eng = _engine()
    worst, runs = 0.0, 0
    for numels in _lists():
        for odd in (True, False):
            for max_norm in (0.5, 1e6, None):
                for targets in (False, True):
                    for zg in (False, True):
                        run = Run(eng, numels, dt, kind, odd, targets, seed=runs)
                        for k in range(3):
                            if k:
                                run.set_grads(_data(numels, dt, 1000 + 3 * runs + k))
                            run.device_step(max_norm=max_norm, zero_grad=zg)
                            r = run.check(max_norm=max_norm, zero_grad=zg)
                            if max_norm is not None:
                                assert (r["coef"] == 1.0) == (max_norm == 1e6), (r["total"], r["coef"])
                        worst = max(worst, run.norm_err)
                        runs += 1
    print(f"{kind} {np.dtype(dt).name}: {runs} runs x 3 steps bit for bit; total norm: max error / bound {worst:.4f}")
    assert worst <= 1.0


def test_each_size_alone():
    """every size as a one-tensor list, both alignments, both dtypes: the ragged last thread, wave and chunk on their own"""
    eng = _engine()
    for n in _numels():
        for dt in DTYPES:
            for odd in (True, False):
                run = Run(eng, [n], dt, "adam", odd, True, seed=n)
                run.device_step(max_norm=0.5, zero_grad=True)
                run.check(max_norm=0.5, zero_grad=True)
                assert run.plan.n_chunks == (n + _chunk() - 1) // _chunk()


def test_a_list_past_one_lap_of_the_final_merge():
    """300 chunks: the head kernel's 256 threads take a second partial (d = 24); 0.3 M elements, PPO's size"""
    eng = _engine()
    c = _chunk()
    numels = [150 * c + 5, 148 * c, 77]
    run = Run(eng, numels, np.float32, "adam", False, False, seed=9)
    assert run.plan.n_chunks == 300 and _depth(300) == 24
    run.device_step(max_norm=0.5)
    run.check(max_norm=0.5)
    print(f"300 chunks: total norm max error / bound {run.norm_err:.4f}")


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_planted_values(dt):
    """zero gradients throughout (total = 0: coefficient 1, v = 0 with g = 0 moves nothing), then +-0.0, subnormals and the largest
    and smallest normal magnitudes planted in gradients and parameters"""
    eng = _engine()
    numels = [65, _chunk() + 1]
    for kind in ("adam", "rmsprop"):
        run = Run(eng, numels, dt, kind, True, True, seed=5)
        run.set_grads([np.zeros(n, dt) for n in numels])
        before = [p.copy() for p in run.h_p]
        run.device_step(max_norm=0.5)
        r = run.check(max_norm=0.5)
        assert r["total"] == 0.0 and r["coef"] == 1.0 and all(_same(a, b) for a, b in zip(before, run.h_p))
        assert all(not s.any() for s in run.h_s1)
        tiny = np.finfo(dt).tiny
        g = _data(numels, dt, 77)
        g[0][:8] = [0.0, -0.0, tiny, -tiny, tiny / 4, -tiny / 8, np.nextafter(dt(0), dt(1)), 1e-30]
        g[1][-4:] = [-0.0, tiny / 2, 1e18, -1e-18]
        run.set_grads(g)
        for max_norm in (None, 0.5):
            run.device_step(max_norm=max_norm, zero_grad=False)
            run.check(max_norm=max_norm)
        # a zero gradient where the second moment is still zero beside a parameter of -0.0: 0 / (0 + eps) keeps the sign of the zero
        run2 = Run(eng, [5], dt, kind, False, False, seed=6, p_data=[np.array([-0.0, 0.0, 1.0, tiny / 2, -tiny], dt)])
        run2.set_grads([np.array([0.0, -0.0, 1.0, 0.0, -1.0], dt)])
        run2.device_step()
        run2.check()


def test_two_runs_give_identical_bits():
    eng = _engine()
    numels = _lists()[2]
    outs = []
    for _ in range(2):
        run = Run(eng, numels, np.float32, "adam", False, True, seed=3)
        for k in range(2):
            run.device_step(max_norm=0.5)
            run.check(max_norm=0.5)
        outs.append((run.fp.dev.cpu().numpy(), run.fq.dev.cpu().numpy(), float(run.plan.norm[0]), [s.cpu().numpy() for s in run.plan.state2]))
    a, b = outs
    assert _same(a[0], b[0]) and _same(a[1], b[1]) and a[2] == b[2] and all(_same(x, y) for x, y in zip(a[3], b[3]))


def test_lr_as_a_device_tensor_and_on_a_side_stream():
    import torch
    eng = _engine()
    run = Run(eng, _lists()[1], np.float64, "adam", True, True, seed=8)
    lr = torch.full((1,), 5e-5, dtype=torch.float64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run.device_step(lr=lr, max_norm=0.5)
        eng.sync()
    torch.cuda.current_stream().wait_stream(side)
    run.check(lr=5e-5, max_norm=0.5)
    lr.fill_(1e-2)
    run.device_step(lr=lr, max_norm=0.5)
    run.check(lr=1e-2, max_norm=0.5)


@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
def test_captured_and_replayed_three_times(kind):
    """the call captured once on a side stream and replayed three times with rewritten gradients and the lr tensor changed in between:
    three restatement steps, the step count and the beta products advancing on the device; the host doubles are kept"""
    import torch
    eng = _engine()
    numels = _lists()[2]
    run = Run(eng, numels, np.float32, kind, False, True, seed=12)
    lr = torch.full((1,), 1e-2, dtype=torch.float64, device="cuda")
    run.device_step(lr=lr, max_norm=0.5, zero_grad=True)              # eager once: code objects are loaded before the capture
    run.check(lr=1e-2, max_norm=0.5, zero_grad=True)
    before = run.fp.dev.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            run.device_step(lr=lr, max_norm=0.5, zero_grad=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(before, run.fp.dev) and run.plan.state.cpu().numpy()[0] == 1.0          # capturing enqueued nothing
    for k, rate in enumerate((1e-2, 5e-5, 3e-3)):
        run.set_grads(_data(numels, np.float32, 200 + k))
        lr.fill_(rate)
        graph.replay()
        run.check(lr=rate, max_norm=0.5, zero_grad=True, sync=False)
    assert run.st["t"] == 4.0
    eng.sync()


@pytest.mark.parametrize("what", ["nan", "inf"])
def test_a_non_finite_gradient(what):
    """propagates as the arithmetic says -- with clipping the total is NaN / Inf and every element follows the restatement; without it
    only the element itself is hit -- and the next sync() raises PTG_E_NONFINITE, once"""
    from rl_ptg_amd import _lib
    from rl_ptg_amd.engine import PtgError
    eng = _engine()
    numels = [65, _chunk() + 1]
    for kind in ("adam", "rmsprop"):
        for max_norm in (0.5, None):
            run = Run(eng, numels, np.float32, kind, False, True, seed=21)
            g = _data(numels, np.float32, 22)
            g[1][1000] = np.nan if what == "nan" else -np.inf
            run.set_grads(g)
            run.device_step(max_norm=max_norm)
            with pytest.raises(PtgError) as ei:
                eng.sync()
            assert ei.value.code == _lib.E_NONFINITE
            eng.sync()                                                  # once
            r = run.check(max_norm=max_norm, nan_ok=True)
            if max_norm is not None:
                assert not np.isfinite(r["total"])
                assert np.isnan(run.h_p[0]).all() if what == "nan" else (run.h_s1[0] == 0).all()      # coef NaN poisons all; coef 0 clears the step
            else:
                assert np.isnan(run.h_p[1][1000]) and np.isfinite(run.h_p[0]).all() and np.isfinite(np.delete(run.h_p[1], 1000)).all()
    run = Run(eng, numels, np.float32, "adam", False, False, seed=23)   # a clean call syncs clean
    run.device_step(max_norm=0.5)
    run.check(max_norm=0.5)


def test_standalone_polyak_update():
    """tau = 1 equals a copy, byte for byte (DQN's hard update); tau = 0.005 equals the restatement; the fused call equals the step
    followed by the standalone call; guards untouched; a plan reused makes no allocation"""
    import torch
    eng = _engine()
    for dt in DTYPES:
        for odd in (True, False):
            numels = _lists()[2]
            fp, fq = Flat(numels, dt, odd, _data(numels, dt, 31)), Flat(numels, dt, odd, _data(numels, dt, 32))
            params, targets = fp.upload(), fq.upload()
            plan = eng.polyak_update(params, targets, TAU)
            eng.sync()
            want = orr.polyak(fp.views(fp.host), fq.views(fq.host), TAU)
            assert _same(fq.dev.cpu().numpy(), fq.expect(want)) and _same(fp.dev.cpu().numpy(), fp.host)
            mem = _allocations()
            assert eng.polyak_update(params, targets, 1.0, plan=plan) is plan
            assert _allocations() == mem
            eng.sync()
            assert _same(fq.dev.cpu().numpy(), fq.expect(fp.views(fp.host)))
            for p, q in zip(params, targets):
                assert torch.equal(p.view(torch.int32 if dt == np.float32 else torch.int64), q.view(torch.int32 if dt == np.float32 else torch.int64))
    a = Run(eng, _lists()[1], np.float32, "adam", True, True, seed=33)
    b = Run(eng, _lists()[1], np.float32, "adam", True, False, seed=33)
    a.device_step(max_norm=0.5)
    b.device_step(max_norm=0.5)
    b_targets = Flat(b.numels, np.float32, True, _data(b.numels, np.float32, 35))
    tq = b_targets.upload()
    eng.polyak_update(b.params, tq, TAU)
    eng.sync()
    assert _same(a.fq.dev.cpu().numpy(), b_targets.dev.cpu().numpy()) and _same(a.fp.dev.cpu().numpy(), b.fp.dev.cpu().numpy())


def test_no_host_synchronisation_no_allocation_and_nothing_else_touched():
    """A condition, not a timing: the stream is busy with milliseconds of fused steps before the calls and still busy when they have
    returned; the calls allocate no device memory.  Afterwards env state, finished ring, vn statistics and a replay cursor equal a
    twin's that made no call."""
    import torch
    from rl_ptg_amd import DeviceReplayBuffer
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    n, T, calls = 65536, 250, 8
    spec, _ = synthetic_spec(scenario=2, operation="OP2", eps_len_d=32)
    engs = []
    for _ in range(2):
        e = HipEngine(spec.consts, spec.tables, spec.markets, n, device=0, out_dtype="float32", obs_layout="sb3_flat")
        e.set_episode_plan(spec.eps_ind, n, n)
        e.set_noise_rng(5)
        e.vn_init()
        e.reset()
        engs.append(e)
    eng, twin = engs
    buf = DeviceReplayBuffer(eng, 2 * n)
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    acts = torch.randint(0, 5, (T, n), dtype=torch.int32, device="cuda", generator=g)
    run = Run(eng, _lists()[2], np.float32, "adam", False, True, seed=41)
    pol = eng.polyak_update(run.params, run.targets, TAU)
    obs, rew, done = eng.alloc_obs(T), torch.empty((T, n), device="cuda"), torch.empty((T, n), dtype=torch.uint8, device="cuda")
    eng.rollout(acts, obs, rew, done)                                # warm: first-launch work is not part of the condition
    twin.rollout(acts)
    run.device_step(max_norm=0.5)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    assert stream.query() is True
    for _ in range(calls):
        eng.rollout(acts, obs, rew, done)
    busy_before = stream.query()
    mem = _allocations()
    run.device_step(max_norm=0.5, zero_grad=True)
    eng.polyak_update(run.params, run.targets, TAU, plan=pol)
    assert _allocations() == mem
    busy_after = stream.query()
    assert busy_before is False, "the rollouts were over before the calls: the check would prove nothing"
    assert busy_after is False, "the stream was idle when the calls had returned: a call waited for the device"
    eng.sync()
    assert float(run.plan.state[0]) == 2.0
    for _ in range(calls):
        twin.rollout(acts)
    twin.sync()
    a, b = eng.state_dict(), twin.state_dict()
    assert _equal_state(a["fields"], b["fields"]) and _equal_state(a["vn"], b["vn"])
    assert buf.cursor() == (0, 0)
    assert len(eng.finished_episodes()[0]) == len(twin.finished_episodes()[0])
    eng.close(); twin.close()


def test_refused_arguments_enqueue_nothing():
    import torch
    from rl_ptg_amd import _lib
    eng = _engine()
    L, h, stream = eng._L, eng._h, eng._stream()
    run = Run(eng, [65, _chunk() + 1], np.float32, "adam", False, True, seed=51)
    plan = run.plan
    plan.workspace.fill_(0x5A)
    torch.cuda.synchronize()
    nan = float("nan")

    def desc(**kw):
        a = dict(kind=_lib.OPTIM_ADAM, flags=_lib.OPTIM_CLIP | _lib.OPTIM_TARGETS | _lib.OPTIM_ZERO_GRAD, dtype=_lib.OUT_F32, n_tensors=2, n_chunks=plan.n_chunks,
                 tensors_dev=plan.tensors_dev.data_ptr(), chunks_dev=plan.chunks_dev.data_ptr(), state_dev=plan.state.data_ptr(), norm_dev=plan.norm.data_ptr(),
                 ws_dev=plan.workspace.data_ptr(), lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, alpha=0.99, tau=0.005, max_norm=0.5)
        a.update(kw)
        return _lib.PtgOptim(**a)

    bad = [desc(kind=3), desc(kind=-1), desc(flags=8), desc(flags=16 | 1), desc(dtype=2), desc(dtype=-1), desc(n_tensors=0), desc(n_tensors=-2),
           desc(n_chunks=0), desc(n_chunks=-1), desc(n_chunks=2 ** 31), desc(tensors_dev=None), desc(chunks_dev=None),
           desc(tensors_dev=plan.tensors_dev.data_ptr() + 4), desc(chunks_dev=plan.chunks_dev.data_ptr() + 2), desc(state_dev=None), desc(ws_dev=None),
           desc(ws_dev=plan.workspace.data_ptr() + 4), desc(norm_dev=None), desc(lr=-1.0), desc(lr=nan), desc(lr=float("inf")), desc(eps=-1.0), desc(eps=nan),
           desc(beta1=1.0), desc(beta1=-0.1), desc(beta2=1.0), desc(beta2=nan), desc(tau=1.5), desc(tau=-0.1), desc(tau=nan), desc(max_norm=-1.0), desc(max_norm=nan),
           desc(kind=_lib.OPTIM_RMSPROP, alpha=-0.5), desc(kind=_lib.OPTIM_RMSPROP, alpha=nan),
           desc(kind=_lib.OPTIM_POLYAK, flags=_lib.OPTIM_CLIP), desc(kind=_lib.OPTIM_POLYAK, flags=_lib.OPTIM_ZERO_GRAD), desc(kind=_lib.OPTIM_POLYAK, flags=0, tau=2.0)]
    for k, ds in enumerate(bad):
        assert L.ptg_optim_step(h, C.byref(ds), stream) == _lib.E_INVALID, k
        assert b"ptg_optim_step" in L.ptg_last_error(h)
        assert torch.cuda.current_stream().query() is True, k
    assert L.ptg_optim_step(h, None, stream) == _lib.E_INVALID and L.ptg_optim_step(None, C.byref(desc()), stream) == _lib.E_INVALID
    assert bool((plan.workspace == 0x5A).all()) and plan.state.cpu().tolist() == [0.0, 1.0, 1.0, 0.0]
    assert _same(run.fp.dev.cpu().numpy(), run.fp.host) and _same(run.fq.dev.cpu().numpy(), run.fq.host) and _same(run.fg.dev.cpu().numpy(), run.fg.host)
    # a span that names no tensor of the table never becomes an address: PTG_E_INDEX, the other chunks are computed
    spans = plan.chunks_dev.clone()
    spans[0, 0] = 7
    rc = L.ptg_optim_step(h, C.byref(desc(kind=_lib.OPTIM_POLYAK, flags=0, chunks_dev=spans.data_ptr())), stream)
    assert rc == 0
    from rl_ptg_amd.engine import PtgError
    with pytest.raises(PtgError) as ei:
        eng.sync()
    assert ei.value.code == _lib.E_INDEX
    eng.sync()
    assert _same(run.fq.views(run.fq.dev.cpu().numpy())[0], run.fq.views(run.fq.host)[0])
    spans = plan.chunks_dev.clone()                                     # an offset that is no multiple of the chunk: the same, for its chunk alone
    spans[1, 1] = 4
    assert L.ptg_optim_step(h, C.byref(desc(kind=_lib.OPTIM_POLYAK, flags=0, chunks_dev=spans.data_ptr())), stream) == 0
    with pytest.raises(PtgError) as ei:
        eng.sync()
    assert ei.value.code == _lib.E_INDEX
    eng.sync()
    lr_t = torch.zeros(1, dtype=torch.float64, device="cuda")
    good = [desc(), desc(flags=0, norm_dev=None, max_norm=nan, tau=nan), desc(kind=_lib.OPTIM_RMSPROP, beta1=nan, beta2=7.0),
            desc(kind=_lib.OPTIM_POLYAK, flags=0, state_dev=None, ws_dev=None, lr=nan, eps=nan, tau=1.0), desc(lr=nan, lr_dev=lr_t.data_ptr())]
    for k, ds in enumerate(good):
        assert L.ptg_optim_step(h, C.byref(ds), stream) == 0, (k, L.ptg_last_error(h))
    eng.sync()


def test_device_optimizer_rebuilds_when_a_gradient_moves_and_raises_under_capture():
    import torch
    from rl_ptg_amd import DeviceOptimizer
    eng = _engine()
    torch.manual_seed(1)
    w = [torch.randn(70, device="cuda", requires_grad=True), torch.randn(3, 5, device="cuda", requires_grad=True)]
    host = [x.detach().cpu().numpy().copy() for x in w]
    opt = DeviceOptimizer(eng, w, kind="rmsprop", lr=7e-4, eps=1e-5, max_grad_norm=0.5)
    with pytest.raises(ValueError):
        opt.step()                                                      # no gradients yet
    s1, st = [np.zeros_like(a) for a in host], orr.new_state()
    plans = []
    for k in range(3):
        opt.zero_grad(set_to_none=True)                                 # the next backward allocates fresh gradients, elsewhere: the plan
        sum((x * x).sum() * (k + 1) for x in w).backward()               # keeps the earlier ones alive
        opt.step()
        plans.append(opt.plan)
        eng.sync()
        grads = [x.grad.cpu().numpy() for x in w]
        r = orr.step("rmsprop", host, grads, s1, None, st, 7e-4, eps=1e-5, alpha=0.99, max_norm=0.5, total=float(opt.grad_norm[0]))
        host, s1 = r["params"], r["state1"]
        for a, x in zip(host, w):
            assert _same(x.detach().cpu().numpy(), a.reshape(x.shape))
    assert plans[0] is not plans[1] and plans[0].state is plans[2].state and float(opt.plan.state[0]) == 3.0
    assert opt.state_dict()["state"][1]["square_avg"].shape == (3, 5) and float(opt.state_dict()["state"][0]["step"]) == 3.0
    # under capture a moved gradient cannot be followed: step() raises before anything is enqueued
    opt.zero_grad(set_to_none=True)
    for x in w:
        x.grad = torch.ones_like(x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    raised, tick = False, torch.zeros(4, device="cuda")
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            tick.add_(1.0)
            try:
                opt.step()
            except RuntimeError as e:
                raised = "capture" in str(e)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert raised and float(opt.plan.state[0]) == 3.0
    opt.step()                                                          # eagerly the tables follow
    eng.sync()
    assert float(opt.plan.state[0]) == 4.0


def test_end_to_end_five_ppo_steps_against_the_restatement_and_a_torch_twin():
    """float64 Linear(40, 64) - ReLU - Linear(64, 6), five steps of ppo_loss + DeviceOptimizer (clip 0.5, Adam eps 1e-5): after each step
    the restatement run on the same read-back gradients gives the same bits; a twin stepped by clip_grad_norm_ + torch.optim.Adam on
    the device stays within the host test's bound times the step count, 1e-12 * max(1, |ref|) * k"""
    import torch
    import policy_loss_restatement as pr
    from rl_ptg_amd import DeviceOptimizer, ppo_loss
    eng = _engine()
    B, A, lr = 203, 5, 3e-4
    torch.manual_seed(7)
    mk = lambda: torch.nn.Sequential(torch.nn.Linear(40, 64), torch.nn.ReLU(), torch.nn.Linear(64, A + 1)).double().cuda()
    net, twin = mk(), mk()
    twin.load_state_dict(net.state_dict())
    obs = torch.randn(B, 40, dtype=torch.float64, device="cuda")
    c = pr.case(B, A, np.float64)
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in c.items()}
    with torch.no_grad():
        out0 = net(obs)
        lp0 = torch.distributions.Categorical(logits=out0[:, :A]).log_prob(d["actions"])
        old_lp = (lp0 - torch.from_numpy(np.random.default_rng(5).uniform(-0.1, 0.1, B)).cuda()).contiguous()
    opt = DeviceOptimizer(eng, net.parameters(), kind="adam", lr=lr, eps=1e-5, max_grad_norm=0.5)
    ref = torch.optim.Adam(twin.parameters(), lr=lr, eps=1e-5)

    def loss_of(m):
        o = m(obs)
        return ppo_loss(eng, o[:, :A], o[:, A], d["actions"], old_lp, d["advantages"], d["returns"], clip_range=pr.CLIP, ent_coef=pr.ENT_COEF, vf_coef=pr.VF_COEF)[0]

    host = [p.detach().cpu().numpy().copy() for p in net.parameters()]
    s1, s2, st = [np.zeros_like(a) for a in host], [np.zeros_like(a) for a in host], orr.new_state()
    worst = 0.0
    for k in range(1, 6):
        opt.zero_grad()
        loss_of(net).backward()
        grads = [p.grad.cpu().numpy().copy() for p in net.parameters()]
        opt.step()
        eng.sync()
        total = float(opt.grad_norm[0])
        _check_norm(total, grads, opt.plan.n_chunks)
        r = orr.step("adam", host, grads, s1, s2, st, lr, betas=(0.9, 0.999), eps=1e-5, max_norm=0.5, total=total)
        host, s1, s2 = r["params"], r["state1"], r["state2"]
        for a, p, m, v in zip(host, net.parameters(), opt.plan.state1, opt.plan.state2):
            assert _same(p.detach().cpu().numpy(), a) and r["coef"] <= 1.0
        assert all(_same(m.cpu().numpy(), a) for m, a in zip(opt.plan.state1, s1)) and all(_same(v.cpu().numpy(), a) for v, a in zip(opt.plan.state2, s2))
        ref.zero_grad()
        loss_of(twin).backward()
        torch.nn.utils.clip_grad_norm_(twin.parameters(), 0.5)
        ref.step()
        for p, q in zip(net.parameters(), twin.parameters()):
            e = ((p.detach() - q.detach()).abs() / (1e-12 * k * torch.clamp(q.detach().abs(), min=1.0))).max()
            worst = max(worst, float(e))
        assert worst <= 1.0, (k, worst)
    print(f"five steps against torch.optim.Adam + clip_grad_norm_ on the device: max error / (bound x step) {worst:.5f}")
