"""ptg_policy_loss_group / ptg_optim_step_group, HipEngine.policy_loss_group / optim_step_group, rl_ptg_amd.ppo_loss_group and
DeviceOptimizerGroup (include/ptg_env.h) on the device.

No tolerance anywhere.  A grouped call is DEFINED as the single calls on its members, so every comparison is against policy_loss /
optim_step on a copy of the same member, through integer views: every bit equal, except that where the single call gives a NaN the
grouped call must give a NaN (payload and sign of a NaN are not part of the contract).

The loss grid is thinned diagonally.  Full: G in {1, 2, 3, 8} x B in {1, 5, 64, 65, 203, 256, 257, 513} x five (kind, flags) x three
heads x two dtypes x {strided, contiguous}.  Run: every (B, (kind, flags)) pair -- 40 cases, B the test's parameter -- with
G = GS[(b + c) % 4], head = HEADS[(b + 2 c) % 3], dtype = f32 if (b + c) % 2 == 0 else f64, and the strided [B][A + 1] actor-critic
layout when c is even (b, c: the indices of B and of (kind, flags)).  Over the 40 cases every G meets every B at least once, every head
every (kind, flags), both dtypes every B, and B = 256 | 257 -- the edge between the one-block path and rows + final -- meet G = 8."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GS = [1, 2, 3, 8]
BS = [1, 5, 64, 65, 203, 256, 257, 513]
CONFIGS = [("ppo", False, False), ("ppo", True, False), ("ppo", True, True), ("ppo", False, True), ("a2c", True, False)]      # kind, NORM_ADV, CLIP_VF
HEADS = [2, 5, "gauss"]
SENTINEL = 7.5
_engines = {}
_spec = []


def _engine(n=6):
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    if n in _engines:
        return _engines[n]
    if not _spec:
        _spec.append(synthetic_spec(scenario=2, operation="OP2", eps_len_d=1, train_steps=200000)[0])
    s = _spec[0]
    eng = HipEngine(s.consts, s.tables, s.markets, n, device=0, out_dtype="float32", obs_layout="sb3_flat")
    eng.set_episode_plan(s.eps_ind, n, n)
    eng.set_noise_rng(seed=4)
    _engines[n] = eng
    return eng


def _bits(t):
    """a device tensor's elements as integers on the host (the logical elements of a strided view)"""
    a = t.detach().contiguous().cpu().numpy()
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(got, want, what=""):
    """bit equality through integer views; a NaN of the single call must meet a NaN"""
    assert got.dtype == want.dtype and got.shape == want.shape, what
    g, w = got.detach().contiguous().cpu().numpy(), want.detach().contiguous().cpu().numpy()
    n = np.isnan(w) if w.dtype.kind == "f" else np.zeros(w.shape, bool)
    assert np.array_equal(np.isnan(g) if g.dtype.kind == "f" else n, n), f"{what}: NaN positions"
    assert np.array_equal(_bits(got)[~n], _bits(want)[~n]), f"{what}: bits"


def _allocations():
    import torch
    return torch.cuda.memory_stats()["allocation.all.allocated"]


def _expect_error(eng, code):
    """the next sync raises PtgError with `code`, once"""
    from rl_ptg_amd.engine import PtgError
    with pytest.raises(PtgError) as ei:
        eng.sync()
    assert ei.value.code == code
    eng.sync()


# ================================================================================================= the loss
def _loss_member(eng, i, B, head, dt, kind, clip_vf, strided, seed):
    """member i's arguments (inputs on the device, every scalar its own) and a maker of fresh outputs, sentinel-filled"""
    import torch
    g = torch.Generator(device="cuda"); g.manual_seed(1000 * seed + i)
    rn = lambda *s: torch.randn(*s, dtype=dt, device="cuda", generator=g)
    gauss = head == "gauss"
    A = 0 if gauss else head
    m = {}
    if gauss:
        both = rn(B, 2)
        m["head_input"], m["values"] = (both[:, 0], both[:, 1]) if strided else (rn(B), rn(B))
        m["actions"], m["log_std"] = rn(B), torch.tensor([-0.3 + 0.1 * i], dtype=dt, device="cuda")
        m["old_log_prob"] = -1.0 + 0.2 * rn(B)
    else:
        ac = rn(B, A + 1)
        m["head_input"], m["values"] = (ac[:, :A], ac[:, A]) if strided else (rn(B, A), rn(B))
        m["actions"] = torch.randint(0, A, (B,), dtype=torch.int64, device="cuda", generator=g)
        m["old_log_prob"] = -float(np.log(A)) + 0.2 * rn(B)
    m["advantages"], m["returns"] = rn(B), rn(B)
    if kind == "a2c":
        del m["old_log_prob"]
    else:
        m["clip_range"] = 0.1 + 0.05 * i
    if clip_vf:
        m["old_values"], m["clip_range_vf"] = m["values"].detach().clone().contiguous() + 0.3 * rn(B), 0.2 + 0.1 * i
    m["ent_coef"], m["vf_coef"] = 0.01 * (i + 1), 0.5 + 0.07 * i

    def outputs():
        full = lambda *s: torch.full(s, SENTINEL, dtype=dt, device="cuda")
        if gauss:
            both = full(B, 2)
            gi, gv = (both[:, 0], both[:, 1]) if strided else (full(B), full(B))
        else:
            ac = full(B, A + 1)
            gi, gv = (ac[:, :A], ac[:, A]) if strided else (full(B, A), full(B))
        return (torch.full((8,), SENTINEL, dtype=torch.float64, device="cuda"), gi, gv, full(1) if gauss else None), eng.policy_loss_workspace(B)
    return m, outputs


def _single(eng, kind, m, out, ws, norm):
    a = dict(m)
    if kind == "a2c":
        a["old_log_prob"] = None
    return eng.policy_loss(kind, a.pop("head_input"), a.pop("values"), a.pop("actions"), a.pop("old_log_prob"), a.pop("advantages"), a.pop("returns"),
                           normalize_advantage=norm, out=out, workspace=ws, **a)


def _compare_loss(eng, G, B, head, dt, kind, norm, clip_vf, strided, seed, plant=None, expect=None):
    """one grouped call against the G single calls on the same inputs and fresh outputs; plant(members) edits the inputs first"""
    import torch
    made = [_loss_member(eng, i, B, head, dt, kind, clip_vf, strided, seed) for i in range(G)]
    if plant:
        plant([m for m, _ in made])
    outs_g, outs_s = [o() for _, o in made], [o() for _, o in made]
    members = [dict(m, out=o, workspace=w) for (m, _), (o, w) in zip(made, outs_g)]
    torch.cuda.synchronize()
    mem = _allocations()
    res = eng.policy_loss_group(kind, members, normalize_advantage=norm)
    assert _allocations() == mem, "out= and workspace= given: nothing is allocated"
    if expect is not None:
        _expect_error(eng, expect)
    else:
        eng.sync()
    singles = []
    for (m, _), (o, w) in zip(made, outs_s):
        singles.append(_single(eng, kind, m, o, w, norm))
        try:
            eng.sync()
        except Exception:
            assert expect is not None
    for i, (r, s) in enumerate(zip(res, singles)):
        tag = f"G={G} B={B} head={head} {dt} {kind} norm={norm} clip_vf={clip_vf} strided={strided} member {i}"
        _same(r.stats, s.stats, tag + " stats")
        _same(r.grad_input, s.grad_input, tag + " grad_input")
        _same(r.grad_values, s.grad_values, tag + " grad_values")
        if head == "gauss":
            _same(r.grad_log_std, s.grad_log_std, tag + " grad_log_std")
        assert r.stats is members[i]["out"][0]
    return res, singles, members


@pytest.mark.parametrize("B", BS)
def test_the_loss_grid_bit_for_bit(B):
    import torch
    eng = _engine()
    b = BS.index(B)
    for c, (kind, norm, clip_vf) in enumerate(CONFIGS):
        G, head, dt = GS[(b + c) % 4], HEADS[(b + 2 * c) % 3], torch.float32 if (b + c) % 2 == 0 else torch.float64
        res, _, _ = _compare_loss(eng, G, B, head, dt, kind, norm, clip_vf, strided=c % 2 == 0, seed=10 * b + c)
        stats = torch.stack([r.stats for r in res]).cpu().numpy()
        assert np.isfinite(stats).all() and (G == 1 or len({s.tobytes() for s in stats}) == G), "the members' scalars and data differ, so must their statistics"


def test_the_thinned_grid_covers_what_the_docstring_says():
    seen = [(GS[(b + c) % 4], HEADS[(b + 2 * c) % 3], (b + c) % 2, b, c) for b in range(len(BS)) for c in range(len(CONFIGS))]
    assert {(g, b) for g, _, _, b, _ in seen} == {(g, b) for g in GS for b in range(len(BS))}
    assert {(h, c) for _, h, _, _, c in seen} == {(h, c) for h in HEADS for c in range(len(CONFIGS))}
    assert {(d, b) for _, _, d, b, _ in seen} == {(d, b) for d in (0, 1) for b in range(len(BS))}
    assert (8, BS.index(256)) in {(g, b) for g, _, _, b, _ in seen} and (8, BS.index(257)) in {(g, b) for g, _, _, b, _ in seen}


def test_a_group_of_one_and_int32_actions_equal_the_single_call():
    import torch
    eng = _engine()
    for B in (5, 257):
        _compare_loss(eng, 1, B, 5, torch.float32, "ppo", True, True, True, seed=77)

    def to_i32(ms):
        for m in ms:
            m["actions"] = m["actions"].to(torch.int32)
    _compare_loss(eng, 3, 65, 5, torch.float32, "ppo", True, False, True, seed=78, plant=to_i32)


@pytest.mark.parametrize("B", [65, 513])
def test_an_action_out_of_range_in_member_1_of_3(B):
    """PTG_E_INDEX once; the row is skipped as the single call skips it, and members 0 and 2 are what their own calls give"""
    import torch
    from rl_ptg_amd import _lib
    eng = _engine()

    def plant(ms):
        ms[1]["actions"][B // 2] = 5
    res, _, _ = _compare_loss(eng, 3, B, 5, torch.float32, "ppo", True, False, True, seed=81, plant=plant, expect=_lib.E_INDEX)
    assert bool((res[1].grad_input[B // 2] == SENTINEL).all())            # never an address: the row's gradients stay as they were
    for i in (0, 2):
        assert bool(torch.isfinite(res[i].stats).all()) and bool(torch.isfinite(res[i].grad_input).all())


@pytest.mark.parametrize("B", [65, 513])
def test_a_nan_advantage_under_norm_adv_in_member_1_of_3(B):
    """A2C, where a row's surrogate gradient is its normalised advantage itself: the moments of member 1 are NaN, so is every row's
    normalised advantage, so its policy gradient and loss are all NaN, and the next sync raises PTG_E_NONFINITE once; members 0 and 2 are
    what their own calls give, finite.  (Under PPO a row whose ratio lies outside the clip range has a zero surrogate gradient whatever
    its advantage: the grid's comparison with the single call covers that.)"""
    import torch
    from rl_ptg_amd import _lib
    eng = _engine()

    def plant(ms):
        ms[1]["advantages"][B // 3] = float("nan")
    res, _, _ = _compare_loss(eng, 3, B, 5, torch.float32, "a2c", True, False, False, seed=82, plant=plant, expect=_lib.E_NONFINITE)
    assert bool(torch.isnan(res[1].grad_input).all()) and bool(torch.isnan(res[1].stats[:2]).all())
    for i in (0, 2):
        assert bool(torch.isfinite(res[i].stats).all()) and bool(torch.isfinite(res[i].grad_input).all()) and bool(torch.isfinite(res[i].grad_values).all())


def test_the_loss_gives_identical_bits_on_two_runs():
    import torch
    eng = _engine()
    a, _, _ = _compare_loss(eng, 3, 513, 5, torch.float32, "a2c", True, False, True, seed=83)
    b, _, _ = _compare_loss(eng, 3, 513, 5, torch.float32, "a2c", True, False, True, seed=83)
    for x, y in zip(a, b):
        _same(x.stats, y.stats), _same(x.grad_input, y.grad_input), _same(x.grad_values, y.grad_values)


# ================================================================================================= the optimiser
NUMELS = [[3], [1, 1025], [1023, 1024, 2049, 1025]]          # 1, 3 and 7 chunks: the grid is 7 wide, members 0 and 1 have surplus workgroups


class Agent:
    """one member's tensors: parameters (member 2: views at odd element offsets of a flat buffer, the element-wise path), targets, and
    the gradients of `steps` steps; twin(): the same data in fresh tensors at the same alignment"""

    def __init__(self, eng, numels, dt, kind, targets, odd, seed, data=None):
        import torch
        self.eng, self.numels, self.dt, self.kind, self.odd = eng, numels, dt, kind, odd
        if data is None:
            g = torch.Generator(device="cuda"); g.manual_seed(seed)
            data = dict(p=[torch.randn(n, dtype=dt, device="cuda", generator=g) for n in numels],
                        q=[torch.randn(n, dtype=dt, device="cuda", generator=g) for n in numels] if targets else None,
                        g=[[torch.randn(n, dtype=dt, device="cuda", generator=g) for n in numels] for _ in range(3)])
        self.data = data
        self.flat = torch.full((sum(numels) + 8 * len(numels) + 8,), SENTINEL, dtype=dt, device="cuda")
        self.params, pos = [], 4
        for n, src in zip(numels, data["p"]):
            start = (pos + 3) // 4 * 4 + (1 if odd else 0)
            v = self.flat[start:start + n]
            v.copy_(src)
            self.params.append(v)
            pos = start + n + 3
        assert all((p.data_ptr() % 16 != 0) == odd for p in self.params)
        self.targets = None if data["q"] is None else [t.clone() for t in data["q"]]
        self.grads = [torch.zeros(n, dtype=dt, device="cuda") for n in numels]
        self.plan = eng.optim_plan(self.params, None if kind == "polyak" else self.grads, kind, targets=self.targets)

    def twin(self):
        return Agent(self.eng, self.numels, self.dt, self.kind, self.targets is not None, self.odd, 0, data=self.data)

    def load_grads(self, k):
        for g, src in zip(self.grads, self.data["g"][k]):
            g.copy_(src)

    def everything(self):
        p = self.plan
        return [("flat", self.flat)] + [(f"grad {k}", g) for k, g in enumerate(self.grads)] + [(f"state1 {k}", s) for k, s in enumerate(p.state1)] + \
               [(f"state2 {k}", s) for k, s in enumerate(p.state2)] + [(f"target {k}", t) for k, t in enumerate(self.targets or [])] + \
               ([] if self.kind == "polyak" else [("state", p.state), ("norm", p.norm)])


def _assert_agents_equal(got, want, what):
    for (name, a), (_, b) in zip(got.everything(), want.everything()):
        _same(a, b, f"{what}: {name}")


OPT_CONFIGS = [("adam", True, True, True), ("adam", False, False, False), ("rmsprop", True, False, True)]      # kind, clip, targets, zero_grad


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("cfg", OPT_CONFIGS, ids=["adam-clip-targets-zero", "adam-plain", "rmsprop-clip-zero"])
def test_the_optimiser_grid_three_steps_bit_for_bit(cfg, dt):
    """members of 1, 3 and 7 chunks (element counts 1, 3, 1023, 1024, 1025, 2049; member 2's parameters at odd offsets of a flat
    buffer); lr from the host in members 0 and 2, from the device in member 1; max_norm such that member 0 clips (0.01), member 1 does
    not (1e6) and member 2 does (0.5); betas, eps, alpha and tau all different.  After each of three steps everything a member owns
    -- parameters and the guards around them, moments, targets, gradients, {t, beta1^t, beta2^t}, the norm -- equals its single twin's"""
    import torch
    kind, clip, targets, zero = cfg
    dt = torch.float32 if dt == "f32" else torch.float64
    eng = _engine()
    agents = [Agent(eng, n, dt, kind, targets, odd=i == 2, seed=300 + i) for i, n in enumerate(NUMELS)]
    assert [a.plan.n_chunks for a in agents] == [1, 3, 7]
    twins = [a.twin() for a in agents]
    lr_dev, lr_dev_twin = (torch.tensor([2e-3], dtype=torch.float64, device="cuda") for _ in range(2))
    lrs = lambda dev: [1e-3, dev, 3e-3]
    betas, eps, alpha = [(0.9, 0.999), (0.8, 0.95), (0.7, 0.9)], [1e-8, 1e-5, 1e-6], [0.99, 0.9, 0.95]
    mgn = [0.01, 1e6, 0.5] if clip else [None] * 3
    tau = [0.005, 0.5, 1.0] if targets else [None] * 3
    torch.cuda.synchronize()
    for k in range(3):
        for a in agents + twins:
            a.load_grads(k)
        mem = _allocations()
        eng.optim_step_group([a.plan for a in agents], lrs(lr_dev), betas=betas, eps=eps, alpha=alpha, max_grad_norm=mgn, tau=tau, zero_grad=zero)
        assert _allocations() == mem
        for i, t in enumerate(twins):
            eng.optim_step(t.plan, lrs(lr_dev_twin)[i], betas=betas[i], eps=eps[i], alpha=alpha[i], max_grad_norm=mgn[i], tau=tau[i], zero_grad=zero)
        eng.sync()
        for i, (a, t) in enumerate(zip(agents, twins)):
            _assert_agents_equal(a, t, f"step {k} member {i}")
            assert float(a.plan.state[0]) == k + 1.0
        if clip:
            norms = [float(a.plan.norm) for a in agents]
            assert norms[0] > 0.01 and norms[1] < 1e6 and norms[2] > 0.5, norms          # members 0 and 2 clip, member 1 does not
        lr_dev.mul_(0.5); lr_dev_twin.mul_(0.5)              # annealed in place: read on the device at every step


def _raw_optim_desc(eng, a, kind, flags, **kw):
    from rl_ptg_amd import _lib
    p = a.plan
    d = dict(kind=kind, flags=flags, dtype=_lib.OUT_F32 if p.params[0].element_size() == 4 else _lib.OUT_F64, n_tensors=len(p.params), n_chunks=p.n_chunks,
             tensors_dev=p.tensors_dev.data_ptr(), chunks_dev=p.chunks_dev.data_ptr(), ws_dev=p.workspace.data_ptr(),
             state_dev=None if p.state is None else p.state.data_ptr(), norm_dev=None if p.norm is None else p.norm.data_ptr(),
             lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, alpha=0.99, tau=0.25, max_norm=0.5)
    d.update(kw)
    return _lib.PtgOptim(**d)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_polyak_members_in_one_launch(dt):
    import torch
    from rl_ptg_amd import _lib
    dt = torch.float32 if dt == "f32" else torch.float64
    eng = _engine()
    agents = [Agent(eng, n, dt, "polyak", True, odd=i == 2, seed=400 + i) for i, n in enumerate(NUMELS)]
    twins = [a.twin() for a in agents]
    taus = [0.005, 0.5, 1.0]
    arr = (_lib.PtgOptim * 3)(*[_raw_optim_desc(eng, a, _lib.OPTIM_POLYAK, 0, tau=t, state_dev=None, norm_dev=None) for a, t in zip(agents, taus)])
    assert eng._L.ptg_optim_step_group(eng._h, arr, 3, eng._stream()) == 0, eng._L.ptg_last_error(eng._h)
    for t, tau in zip(twins, taus):
        eng.polyak_update(t.params, t.targets, tau, plan=t.plan)
    eng.sync()
    for i, (a, t) in enumerate(zip(agents, twins)):
        _assert_agents_equal(a, t, f"member {i}")
    _same(agents[2].targets[2], agents[2].params[2], "tau = 1 is a copy")


def test_a_nan_gradient_in_member_1():
    """member 1's total norm is NaN: PTG_E_NONFINITE once, member 1 as its single call leaves it; members 0 and 2 as their single steps"""
    import torch
    from rl_ptg_amd import _lib
    eng = _engine()
    agents = [Agent(eng, n, torch.float32, "adam", False, odd=i == 2, seed=500 + i) for i, n in enumerate(NUMELS)]
    agents[1].data["g"][0][1][1000] = float("nan")
    twins = [a.twin() for a in agents]
    for a in agents + twins:
        a.load_grads(0)
    eng.optim_step_group([a.plan for a in agents], 1e-3, max_grad_norm=0.5, zero_grad=True)
    _expect_error(eng, _lib.E_NONFINITE)
    for i, t in enumerate(twins):
        eng.optim_step(t.plan, 1e-3, max_grad_norm=0.5, zero_grad=True)
        if i == 1:
            _expect_error(eng, _lib.E_NONFINITE)
        else:
            eng.sync()
    for i, (a, t) in enumerate(zip(agents, twins)):
        _assert_agents_equal(a, t, f"member {i}")
    assert bool(torch.isnan(agents[1].plan.norm).all()) and bool(torch.isnan(agents[1].params[1]).all())
    assert all(bool(torch.isfinite(agents[i].flat).all()) for i in (0, 2))


def test_a_span_with_a_bad_tensor_index_in_member_2():
    """the chunk is skipped -- never an address -- and PTG_E_INDEX is raised once; every other chunk of every member is computed"""
    import torch
    from rl_ptg_amd import _lib
    eng = _engine()
    agents = [Agent(eng, n, torch.float32, "adam", False, odd=i == 2, seed=600 + i) for i, n in enumerate(NUMELS)]
    twins = [a.twin() for a in agents]
    for a in (agents[2], twins[2]):
        a.plan.chunks_dev[1, 0] = 99                          # chunk 1: tensor 1 (1024 elements) of member 2
    for a in agents + twins:
        a.load_grads(0)
    eng.optim_step_group([a.plan for a in agents], [1e-3, 2e-3, 3e-3], max_grad_norm=None, zero_grad=True)
    _expect_error(eng, _lib.E_INDEX)
    for i, t in enumerate(twins):
        eng.optim_step(t.plan, [1e-3, 2e-3, 3e-3][i], max_grad_norm=None, zero_grad=True)
        if i == 2:
            _expect_error(eng, _lib.E_INDEX)
        else:
            eng.sync()
    for i, (a, t) in enumerate(zip(agents, twins)):
        _assert_agents_equal(a, t, f"member {i}")
    _same(agents[2].params[1], agents[2].data["p"][1], "the skipped chunk's parameters")
    _same(agents[2].grads[1], agents[2].data["g"][0][1], "the skipped chunk's gradients")
    assert not torch.equal(agents[2].params[0], agents[2].data["p"][0]) and not torch.equal(agents[2].params[2], agents[2].data["p"][2])


def test_the_optimiser_gives_identical_bits_on_two_runs():
    import torch
    eng = _engine()
    runs = []
    for _ in range(2):
        agents = [Agent(eng, n, torch.float32, "adam", True, odd=i == 2, seed=700 + i) for i, n in enumerate(NUMELS)]
        for a in agents:
            a.load_grads(0)
        eng.optim_step_group([a.plan for a in agents], 1e-3, max_grad_norm=0.5, tau=0.005)
        eng.sync()
        runs.append(agents)
    for a, b in zip(*runs):
        _assert_agents_equal(a, b, "two runs")


# ================================================================================================= together
def test_three_agents_eager_captured_and_replayed_against_single_twins():
    """Three agents of two nets each (40 -> 32 -> 5 and 40 -> 32 -> 1, B = 21) in ONE TrainMLPGroup of six networks: ppo_loss_group -> one
    torch.autograd.backward -> DeviceOptimizerGroup.step() with zero_grad.  One eager step, a capture on a side stream (at the default
    hardware-queue setting), three replays with the batch tensors rewritten in place.  After every step every parameter and every Adam
    state of every agent equals, bit for bit, a twin agent's that steps singly: its own TrainMLPGroup of two nets, ppo_loss, DeviceOptimizer."""
    import torch
    from torch import nn
    from rl_ptg_amd import DeviceOptimizer, DeviceOptimizerGroup, TrainMLPGroup, ppo_loss, ppo_loss_group
    eng = _engine(6)
    G, B, F, A = 3, 21, 40, 5
    lr, clip, ent, vf, mgn = [3e-3, 1e-3, 2e-3], [0.2, 0.1, 0.3], [0.01, 0.0, 0.02], [0.5, 0.4, 0.6], [0.5, 0.05, 5.0]

    def nets(seed):
        torch.manual_seed(seed)
        return (nn.Sequential(nn.Linear(F, 32), nn.Tanh(), nn.Linear(32, A)).cuda(), nn.Sequential(nn.Linear(F, 32), nn.Tanh(), nn.Linear(32, 1)).cuda())

    def optimizer(params, i):
        for p in params:
            p.grad = torch.zeros_like(p)
        return DeviceOptimizer(eng, params, kind="adam", lr=lr[i], eps=1e-5, max_grad_norm=mgn[i], zero_grad=True)

    gen = torch.Generator(device="cuda"); gen.manual_seed(5)

    def batch():
        return dict(obs=torch.randn(B, F, device="cuda", generator=gen), actions=torch.randint(0, A, (B,), device="cuda", generator=gen),
                    old_log_prob=-1.6 + 0.1 * torch.randn(B, device="cuda", generator=gen), advantages=torch.randn(B, device="cuda", generator=gen),
                    returns=torch.randn(B, device="cuda", generator=gen))
    steps = [[batch() for _ in range(G)] for _ in range(5)]                  # per step, per agent
    static = [{k: v.clone() for k, v in b.items()} for b in steps[0]]

    pairs = [nets(40 + i) for i in range(G)]
    grp = TrainMLPGroup(eng, [m for pair in pairs for m in pair], batch=B)
    per_agent = [[p for m in pair for p in (m[0].weight, m[0].bias, m[2].weight, m[2].bias)] for pair in pairs]
    opts = [optimizer(per_agent[i], i) for i in range(G)]
    ogrp = DeviceOptimizerGroup(eng, opts)
    wss = [eng.policy_loss_workspace(B) for _ in range(G)]

    def grouped_step():
        outs = grp([s["obs"] for s in static for _ in range(2)])
        members = [dict(head_input=outs[2 * i], values=outs[2 * i + 1], actions=static[i]["actions"], old_log_prob=static[i]["old_log_prob"],
                        advantages=static[i]["advantages"], returns=static[i]["returns"], workspace=wss[i]) for i in range(G)]
        losses, _ = ppo_loss_group(eng, members, clip_range=clip, ent_coef=ent, vf_coef=vf)
        torch.autograd.backward(losses)
        ogrp.step()

    class Twin:
        def __init__(self, i):
            self.i, self.pair = i, nets(40 + i)
            self.grp = TrainMLPGroup(eng, list(self.pair), batch=B)
            self.params = self.grp.parameters()
            self.opt = optimizer(self.params, i)
            self.ws = eng.policy_loss_workspace(B)

        def __call__(self, b):
            logits, values = self.grp(b["obs"])
            loss, _ = ppo_loss(eng, logits, values, b["actions"], b["old_log_prob"], b["advantages"], b["returns"], clip_range=clip[self.i], ent_coef=ent[self.i],
                               vf_coef=vf[self.i], workspace=self.ws)
            loss.backward()
            self.opt.step()
    twins = [Twin(i) for i in range(G)]

    def check(step):
        torch.cuda.synchronize()
        for i in range(G):
            for k, (p, q) in enumerate(zip(per_agent[i], twins[i].params)):
                _same(p, q, f"step {step} agent {i} parameter {k}")
            a, b = opts[i].plan, twins[i].opt.plan
            for k, (x, y) in enumerate(zip(a.state1 + a.state2 + [a.state, a.norm], b.state1 + b.state2 + [b.state, b.norm])):
                _same(x, y, f"step {step} agent {i} state {k}")
            assert all(not bool(p.grad.any()) for p in per_agent[i])
    start = [p.detach().clone() for ps in per_agent for p in ps]
    grouped_step()                                           # the eager step
    for i, t in enumerate(twins):
        t(steps[0][i])
    check(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            grouped_step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert float(opts[0].plan.state[0]) == 1.0               # capturing ran nothing
    for step in range(1, 4):
        for i in range(G):
            for k, v in steps[step][i].items():
                static[i][k].copy_(v)
        graph.replay()
        for i, t in enumerate(twins):
            t(steps[step][i])
        check(step)
    assert [float(o.plan.state[0]) for o in opts] == [4.0] * G
    assert all(not torch.equal(a, p.detach()) and bool(torch.isfinite(p).all()) for a, p in zip(start, [p for ps in per_agent for p in ps]))
    norms = [float(n) for n in ogrp.grad_norms]
    assert len(set(norms)) == G and all(np.isfinite(norms))
    # a member stays usable alone, and a .grad that moved raises under capture with the member named
    opts[1].step()
    assert float(opts[1].plan.state[0]) == 5.0
    per_agent[2][0].grad = torch.zeros_like(per_agent[2][0])
    side.wait_stream(torch.cuda.current_stream())
    g2 = torch.cuda.CUDAGraph()
    raised, tick = "", torch.zeros(4, device="cuda")
    with torch.cuda.stream(side):
        with torch.cuda.graph(g2, stream=side):
            tick.add_(1.0)
            try:
                ogrp.step()
            except RuntimeError as e:
                raised = str(e)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert "member 2" in raised and "capture" in raised and [float(o.plan.state[0]) for o in opts] == [4.0, 5.0, 4.0]
    ogrp.step()                                              # eagerly member 2's tables follow, its state is kept
    eng.sync()
    assert [float(o.plan.state[0]) for o in opts] == [5.0, 6.0, 5.0]


# ================================================================================================= runtime guarantees
def test_no_host_synchronisation_no_allocation_and_nothing_else_touched():
    """A condition, not a timing (as tests/test_optim.py checks the single call): the stream is busy with milliseconds of fused steps
    before the two grouped calls and still busy when they have returned, and they allocate no device memory.  Afterwards env state, vn
    statistics and a replay cursor equal a twin's that made no call."""
    import torch
    from rl_ptg_amd import DeviceReplayBuffer
    from rl_ptg_amd.engine import HipEngine
    from rl_ptg_amd.prep import synthetic_spec
    from test_optim import _equal_state
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
    agents = [Agent(eng, nm, torch.float32, "adam", True, odd=i == 2, seed=800 + i) for i, nm in enumerate(NUMELS)]
    made = [_loss_member(eng, i, 513, 5, torch.float32, "ppo", True, True, 90) for i in range(3)]
    members = [dict(m, out=o, workspace=w) for (m, _), (o, w) in zip(made, [o() for _, o in made])]
    step = lambda: (eng.policy_loss_group("ppo", members, normalize_advantage=True),
                    eng.optim_step_group([a.plan for a in agents], 1e-3, max_grad_norm=0.5, tau=0.005, zero_grad=True))
    obs, rew, done = eng.alloc_obs(T), torch.empty((T, n), device="cuda"), torch.empty((T, n), dtype=torch.uint8, device="cuda")
    eng.rollout(acts, obs, rew, done)                                # warm: first-launch work is not part of the condition
    twin.rollout(acts)
    step()
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    assert stream.query() is True
    for _ in range(calls):
        eng.rollout(acts, obs, rew, done)
    busy_before = stream.query()
    mem = _allocations()
    step()
    assert _allocations() == mem
    busy_after = stream.query()
    assert busy_before is False, "the rollouts were over before the calls: the check would prove nothing"
    assert busy_after is False, "the stream was idle when the calls had returned: a call waited for the device"
    eng.sync()
    assert [float(a.plan.state[0]) for a in agents] == [2.0] * 3
    for _ in range(calls):
        twin.rollout(acts)
    twin.sync()
    a, b = eng.state_dict(), twin.state_dict()
    assert _equal_state(a["fields"], b["fields"]) and _equal_state(a["vn"], b["vn"])
    assert buf.cursor() == (0, 0)
    eng.close(); twin.close()


def test_c_level_refusals_enqueue_nothing():
    """every refusal with the stream idle afterwards and every output untouched; the text names the member, or the field and the two members"""
    import torch
    from rl_ptg_amd import _lib
    eng = _engine()
    L, h, stream = eng._L, eng._h, eng._stream()
    B, A = 65, 5
    made = [_loss_member(eng, i, B, A, torch.float32, "ppo", True, True, 95) for i in range(3)]
    outs = [o() for _, o in made]

    def loss_desc(i, **kw):
        m, (o, w) = made[i][0], outs[i]
        d = dict(kind=_lib.LOSS_PPO, head=_lib.HEAD_CATEGORICAL, flags=_lib.LOSS_NORM_ADV | _lib.LOSS_CLIP_VF, n_actions=A, in_dtype=_lib.OUT_F32, act_kind=_lib.ACT_I64,
                 batch=B, in_dev=m["head_input"].data_ptr(), in_s_n=A + 1, val_dev=m["values"].data_ptr(), val_s_n=A + 1, act_dev=m["actions"].data_ptr(),
                 old_logp_dev=m["old_log_prob"].data_ptr(), adv_dev=m["advantages"].data_ptr(), ret_dev=m["returns"].data_ptr(), old_val_dev=m["old_values"].data_ptr(),
                 clip_range=0.2, clip_range_vf=0.2, ent_coef=0.01, vf_coef=0.5, stats_dev=o[0].data_ptr(), grad_in_dev=o[1].data_ptr(), g_s_n=A + 1,
                 grad_val_dev=o[2].data_ptr(), gv_s_n=A + 1, ws_dev=w.data_ptr())
        d.update(kw)
        return _lib.PtgLoss(**d)
    for _, w in outs:
        w.fill_(0x5A)
    torch.cuda.synchronize()
    arr = lambda T, ds: (T * len(ds))(*ds)
    L3 = lambda **kw2: [loss_desc(0), loss_desc(1), loss_desc(2, **kw2)]
    bad = [
        (L3(), 0, b"n_members 0 outside"), (L3() * 3, 9, b"n_members 9 outside"), (L3(), -1, b"n_members -1 outside"),
        (L3(batch=0), 3, b"member 2: batch 0 outside"), (L3(in_dev=None), 3, b"member 2: null input"), (L3(ws_dev=None), 3, b"member 2: ws_dev is null"),
        (L3(clip_range=-1.0), 3, b"member 2: clip_range is negative"), (L3(n_actions=33, in_s_n=40, g_s_n=40), 3, b"member 2: n_actions outside"),
        ([loss_desc(0), loss_desc(1, kind=7), loss_desc(2)], 3, b"member 1: unknown kind 7"),
        (L3(kind=_lib.LOSS_A2C), 3, b"members 0 and 2 disagree in kind: 0 and 1"), (L3(flags=_lib.LOSS_NORM_ADV), 3, b"members 0 and 2 disagree in flags: 3 and 1"),
        (L3(head=_lib.HEAD_GAUSSIAN, log_std_dev=made[0][0]["advantages"].data_ptr()), 3, b"members 0 and 2 disagree in head"),
        (L3(n_actions=4), 3, b"members 0 and 2 disagree in n_actions: 5 and 4"), (L3(in_dtype=_lib.OUT_F64), 3, b"members 0 and 2 disagree in in_dtype"),
        (L3(act_kind=_lib.ACT_I32), 3, b"members 0 and 2 disagree in act_kind"), (L3(batch=64), 3, b"members 0 and 2 disagree in batch: 65 and 64"),
        (L3(stats_dev=outs[0][0][0].data_ptr()), 3, b"members 0 and 2 share stats_dev"), (L3(ws_dev=outs[1][1].data_ptr()), 3, b"members 1 and 2 share ws_dev"),
        (L3(grad_in_dev=outs[0][0][1].data_ptr()), 3, b"members 0 and 2 share grad_in_dev"), (L3(grad_val_dev=outs[1][0][2].data_ptr()), 3, b"members 1 and 2 share grad_val_dev"),
    ]
    for k, (ds, n, text) in enumerate(bad):
        assert L.ptg_policy_loss_group(h, arr(_lib.PtgLoss, ds), n, stream) == _lib.E_INVALID, k
        err = L.ptg_last_error(h)
        assert err.startswith(b"ptg_policy_loss_group: ") and text in err, (k, err)
        assert torch.cuda.current_stream().query() is True, k
    assert L.ptg_policy_loss_group(h, None, 3, stream) == _lib.E_INVALID and b"null descriptor array" in L.ptg_last_error(h)
    assert L.ptg_policy_loss_group(None, arr(_lib.PtgLoss, L3()), 3, stream) == _lib.E_INVALID
    for o, w in outs:
        assert bool((w == 0x5A).all()) and all(bool((t == SENTINEL).all()) for t in o[:3])
    # the single entry's words are the shared checker's, unchanged
    assert L.ptg_policy_loss(h, C.byref(loss_desc(0, batch=0)), stream) == _lib.E_INVALID
    assert L.ptg_last_error(h) == b"ptg_policy_loss: batch 0 outside [1, 2^31]"
    assert L.ptg_policy_loss_group(h, arr(_lib.PtgLoss, L3()), 3, stream) == 0, L.ptg_last_error(h)
    eng.sync()

    agents = [Agent(eng, nm, torch.float32, "adam", True, odd=i == 2, seed=900 + i) for i, nm in enumerate(NUMELS)]
    for a in agents:
        a.load_grads(0)
        a.plan.workspace.fill_(0x5A)
    before = [[(n_, t.clone()) for n_, t in a.everything()] for a in agents]
    torch.cuda.synchronize()
    flags = _lib.OPTIM_CLIP | _lib.OPTIM_TARGETS | _lib.OPTIM_ZERO_GRAD
    od = lambda i, **kw: _raw_optim_desc(eng, agents[i], kw.pop("kind", _lib.OPTIM_ADAM), kw.pop("flags", flags), **kw)
    O3 = lambda **kw2: [od(0), od(1), od(2, **kw2)]
    bad = [
        (O3(), 0, b"n_members 0 outside"), (O3() * 3, 9, b"n_members 9 outside"),
        (O3(n_chunks=0), 3, b"member 2: n_chunks 0 outside"), (O3(state_dev=None), 3, b"member 2: null state_dev"), (O3(lr=-1.0), 3, b"member 2: lr is negative"),
        ([od(0), od(1, tau=2.0), od(2)], 3, b"member 1: tau outside"), (O3(max_norm=float("nan")), 3, b"member 2: max_norm is negative or NaN"),
        (O3(kind=_lib.OPTIM_RMSPROP), 3, b"members 0 and 2 disagree in kind: 0 and 1"), (O3(flags=_lib.OPTIM_CLIP), 3, b"members 0 and 2 disagree in flags: 7 and 1"),
        (O3(dtype=_lib.OUT_F64), 3, b"members 0 and 2 disagree in dtype: 0 and 1"),
        (O3(state_dev=agents[0].plan.state.data_ptr()), 3, b"members 0 and 2 share state_dev"), (O3(norm_dev=agents[1].plan.norm.data_ptr()), 3, b"members 1 and 2 share norm_dev"),
        (O3(ws_dev=agents[0].plan.workspace.data_ptr()), 3, b"members 0 and 2 share ws_dev"),
    ]
    for k, (ds, n, text) in enumerate(bad):
        assert L.ptg_optim_step_group(h, arr(_lib.PtgOptim, ds), n, stream) == _lib.E_INVALID, k
        err = L.ptg_last_error(h)
        assert err.startswith(b"ptg_optim_step_group: ") and text in err, (k, err)
        assert torch.cuda.current_stream().query() is True, k
    assert L.ptg_optim_step_group(h, None, 3, stream) == _lib.E_INVALID and L.ptg_optim_step_group(None, arr(_lib.PtgOptim, O3()), 3, stream) == _lib.E_INVALID
    for a, snap in zip(agents, before):
        assert bool((a.plan.workspace == 0x5A).all())
        for (name, t), (_, s) in zip(a.everything(), snap):
            _same(t, s, "untouched " + name)
    assert L.ptg_optim_step(h, C.byref(od(0, n_chunks=0)), stream) == _lib.E_INVALID
    assert L.ptg_last_error(h) == b"ptg_optim_step: n_chunks 0 outside [1, 2^31)"
    assert L.ptg_optim_step_group(h, arr(_lib.PtgOptim, O3()), 3, stream) == 0, L.ptg_last_error(h)
    eng.sync()
