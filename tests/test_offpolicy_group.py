"""ptg_td_loss_group / ptg_actor_loss_group / ptg_rsample_group / ptg_rsample_backward_group, HipEngine.td_loss_group / actor_loss_group /
rsample_group / rsample_backward_group / smooth_target_action_group and rl_ptg_amd's *_group autograd front ends (include/ptg_env.h;
DESIGN.md section 27) on the device.

No tolerance anywhere.  A grouped call is DEFINED as the single calls on its members, so every comparison is against td_loss / actor_loss /
rsample / rsample_backward / smooth_target_action on the same member's data in fresh tensors of the same layout, through integer views:
every bit equal, except that where the single call gives a NaN the grouped call must give a NaN (payload and sign of a NaN are not part
of the contract).

The loss grid is thinned diagonally.  Full: G in {1, 2, 3, 8} x B in {1, 5, 64, 65, 256, 257, 513} x the 13 kinds of CONFIGS x two Q
dtypes x two reward dtypes x two done dtypes x {strided, contiguous} x {target written or not}.  Run: every (B, kind) pair -- 91 cases, B
the test's parameter -- with, b and c being the indices of B and of the kind,
    G = GS[(b + c) % 4], Q dtype f64 if (b + c // 2) % 2 else f32, strided if (b + c // 3) % 2 == 0,
    reward dtype f64 if (b + c // 4) % 2 else f32, done dtype f64 if (b + c // 5) % 2 else f32, the target written if (b + c // 3) % 2.
test_the_thinned_grid_covers_what_the_docstring_says asserts what that covers: every B meets every kind and every G; every kind meets
both Q dtypes and both layouts; every G meets both Q dtypes, both layouts and, in the TD loss, a written and an unwritten target; both
reward and both done dtypes appear; B = 256 | 257 -- the edge between the one-block path and rows + final -- meet G = 8."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GS = [1, 2, 3, 8]
BS = [1, 5, 64, 65, 256, 257, 513]
# (op, kind, what varies)
CONFIGS = [("td", "dqn", dict(A=2, act="i32")), ("td", "dqn", dict(A=5, act="i64")), ("td", "td3", dict(K=1)), ("td", "td3", dict(K=4)),
           ("td", "sac", dict(K=2, alpha="mixed")), ("td", "sac", dict(K=2, alpha="log")),
           ("al", "sac", dict(K=1, alpha="mixed")), ("al", "sac", dict(K=2, alpha="log", ec=True)), ("al", "sac", dict(K=2, alpha="log")),
           ("al", "tqc", dict(K=2, Q=1, alpha="mixed")), ("al", "tqc", dict(K=2, Q=25, alpha="log", ec=True)), ("al", "td3", dict()), ("al", "ent_coef", dict())]
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
    a = t.detach().contiguous().cpu().numpy()
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(got, want, what=""):
    """bit equality through integer views; a NaN of the single call must meet a NaN"""
    assert got.dtype == want.dtype and got.shape == want.shape, what
    g, w = got.detach().contiguous().cpu().numpy(), want.detach().contiguous().cpu().numpy()
    n = np.isnan(w) if w.dtype.kind == "f" else np.zeros(w.shape, bool)
    assert np.array_equal(np.isnan(g) if g.dtype.kind == "f" else n, n), f"{what}: NaN positions"
    assert np.array_equal(_bits(got)[~n], _bits(want)[~n]), f"{what}: bits"


def _flat(res):
    """(name, tensor) of every tensor a result holds: a namedtuple's fields, lists spread, None left out; a bare tensor as itself"""
    if not isinstance(res, tuple):
        return [("out", res)]
    out = []
    for name, v in zip(getattr(res, "_fields", range(len(res))), res):
        for k, t in enumerate(v if isinstance(v, (list, tuple)) else [v]):
            if t is not None:
                out.append((f"{name}[{k}]", t))
    return out


def _same_results(got, want, tag):
    a, b = _flat(got), _flat(want)
    assert [n for n, _ in a] == [n for n, _ in b], tag
    for (name, x), (_, y) in zip(a, b):
        _same(x, y, f"{tag} {name}")


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


def _dt(f64):
    import torch
    return torch.float64 if f64 else torch.float32


# ================================================================================================= the members of the two losses
def _columns(rn, full, B, K, strided, fill=False):
    """K critic outputs [B]: the columns of one [B, K] tensor, or K tensors"""
    mk = full if fill else rn
    if strided:
        wide = mk(B, K + 1)
        return [wide[:, k] for k in range(K)]
    return [mk(B) for _ in range(K)]


def _alpha(m, i, form, name="ent_coef"):
    """every member its own alpha: a host float in the even members and a device scalar in the odd ones ("mixed"), or log alpha"""
    import torch
    if form == "log":
        m["log_ent_coef"] = torch.tensor([-1.0 - 0.1 * i], dtype=torch.float64, device="cuda")
    elif i % 2:
        m[name] = torch.tensor([0.2 + 0.05 * i], dtype=torch.float64, device="cuda")
    else:
        m[name] = 0.2 + 0.05 * i


def _member(eng, op, kind, v, i, B, q64, strided, rew64, done64, want_y, seed):
    """member i's arguments of td_loss / actor_loss (inputs on the device, every scalar its own) and a maker of fresh outputs,
    sentinel-filled, in the inputs' layout"""
    import torch
    dt = _dt(q64)
    g = torch.Generator(device="cuda"); g.manual_seed(1000 * seed + i)
    rn = lambda *s: torch.randn(*s, dtype=dt, device="cuda", generator=g)
    full = lambda *s: torch.full(s, SENTINEL, dtype=dt, device="cuda")
    stats = lambda: torch.full((8,), SENTINEL, dtype=torch.float64, device="cuda")
    m = {}
    if op == "td":
        dqn, A, K = kind == "dqn", v.get("A", 0), v.get("K", 1)
        if dqn:
            wide = lambda mk: mk(B, A + 1)[:, :A] if strided else mk(B, A)
            m["q"], m["next_q"] = wide(rn), wide(rn)
            m["actions"] = torch.randint(0, A, (B,), dtype=torch.int32 if v["act"] == "i32" else torch.int64, device="cuda", generator=g)
        else:
            m["q"], m["next_q"] = _columns(rn, full, B, K, strided), _columns(rn, full, B, K, strided)
        m["rewards"] = torch.randn(B, dtype=_dt(rew64), device="cuda", generator=g)
        m["dones"] = (torch.rand(B, device="cuda", generator=g) < 0.3).to(_dt(done64))
        m["gamma"] = 0.9 + 0.01 * i
        if kind == "sac":
            m["next_log_prob"] = -1.0 + 0.3 * rn(B)
            _alpha(m, i, v["alpha"])
        m["want_target"] = want_y

        def outputs():
            gq = (full(B, A + 1)[:, :A] if strided else full(B, A)) if dqn else _columns(rn, full, B, K, strided, fill=True)
            return (stats(), gq, full(B) if want_y else None), eng.td_loss_workspace(B)
        return m, outputs
    K, Q = v.get("K", 1), v.get("Q", 1)
    if kind == "sac":
        m["q"] = _columns(rn, full, B, K, strided)
    elif kind == "tqc":
        m["q"] = rn(B, K + 1, Q)[:, :K] if strided else [rn(B, Q) for _ in range(K)]
    elif kind == "td3":
        m["q"] = rn(B, 2)[:, 0] if strided else rn(B)
    if kind != "td3":
        m["log_prob"] = -1.0 + 0.3 * rn(B)
        _alpha(m, i, "log" if kind == "ent_coef" else v["alpha"])
    if kind == "ent_coef" or v.get("ec"):
        m["target_entropy"] = -1.0 - 0.1 * i

    def outputs():
        gq = None
        if kind == "sac":
            gq = _columns(rn, full, B, K, strided, fill=True)
        elif kind == "tqc":
            gq = full(B, K + 1, Q)[:, :K] if strided else [full(B, Q) for _ in range(K)]
        elif kind == "td3":
            gq = full(B, 2)[:, 0] if strided else full(B)
        glp = full(B) if kind in ("sac", "tqc") else None
        gla = torch.full((1,), SENTINEL, dtype=torch.float64, device="cuda") if "target_entropy" in m else None
        return (stats(), gq, glp, gla), eng.actor_loss_workspace(B)
    return m, outputs


def _single_loss(eng, op, kind, m, out, ws):
    a = dict(m)
    if op == "td":
        return eng.td_loss(kind, a.pop("q"), a.pop("next_q"), a.pop("rewards"), a.pop("dones"), a.pop("gamma"), out=out, workspace=ws, **a)
    return eng.actor_loss(kind, out=out, workspace=ws, **a)


def _compare_loss(eng, c, G, B, q64=False, strided=True, rew64=False, done64=False, want_y=False, seed=0, plant=None, expect=None):
    """one grouped call against the G single calls on the same data and fresh outputs; plant(members) edits the inputs of both first"""
    import torch
    op, kind, v = CONFIGS[c]
    sides = []
    for _ in range(2):                                       # the grouped call's members, then the single calls': the same data in fresh tensors
        made = [_member(eng, op, kind, v, i, B, q64, strided, rew64, done64, want_y, seed) for i in range(G)]
        if plant:
            plant([m for m, _ in made])
        sides.append([(m, *o()) for m, o in made])
    members = [dict(m, out=o, workspace=w) for m, o, w in sides[0]]
    torch.cuda.synchronize()
    mem = _allocations()
    res = eng.td_loss_group(kind, members) if op == "td" else eng.actor_loss_group(kind, members)
    assert _allocations() == mem, "out= and workspace= given: nothing is allocated"
    if expect is not None:
        _expect_error(eng, expect)
    else:
        eng.sync()
    singles = []
    for m, o, w in sides[1]:
        singles.append(_single_loss(eng, op, kind, m, o, w))
        try:
            eng.sync()
        except Exception:
            assert expect is not None
    for i, (r, s) in enumerate(zip(res, singles)):
        _same_results(r, s, f"{op} {kind} {v} G={G} B={B} f64={q64} strided={strided} member {i}")
        assert r.stats is members[i]["out"][0]
    return res, members


def _thin(b, c):
    return dict(G=GS[(b + c) % 4], q64=(b + c // 2) % 2 == 1, strided=(b + c // 3) % 2 == 0, rew64=(b + c // 4) % 2 == 1, done64=(b + c // 5) % 2 == 1,
                want_y=(b + c // 3) % 2 == 1)


@pytest.mark.parametrize("B", BS)
def test_the_loss_grid_bit_for_bit(B):
    import torch
    eng = _engine()
    b = BS.index(B)
    for c in range(len(CONFIGS)):
        t = _thin(b, c)
        res, _ = _compare_loss(eng, c, B=B, seed=20 * b + c, **t)
        stats = torch.stack([r.stats for r in res]).cpu().numpy()
        assert np.isfinite(stats).all() and not (stats == SENTINEL).any()
        assert t["G"] == 1 or len({s.tobytes() for s in stats}) == t["G"], "the members' scalars and data differ, so must their statistics"


def test_the_thinned_grid_covers_what_the_docstring_says():
    nb, nc = len(BS), len(CONFIGS)
    seen = [(b, c, _thin(b, c)) for b in range(nb) for c in range(nc)]
    assert len(seen) == 91 and {(b, c) for b, c, _ in seen} == {(b, c) for b in range(nb) for c in range(nc)}          # every B meets every kind
    assert {(t["G"], b) for b, _, t in seen} == {(g, b) for g in GS for b in range(nb)}
    assert {(t["q64"], c) for _, c, t in seen} == {(d, c) for d in (False, True) for c in range(nc)}
    assert {(t["strided"], c) for _, c, t in seen} == {(s, c) for s in (False, True) for c in range(nc)}
    assert {(t["G"], t["q64"]) for _, _, t in seen} == {(g, d) for g in GS for d in (False, True)}                     # G = 8 in float32 and in float64
    assert {(t["G"], t["strided"]) for _, _, t in seen} == {(g, s) for g in GS for s in (False, True)}
    td = [t for _, c, t in seen if CONFIGS[c][0] == "td"]
    assert {(t["G"], t["want_y"]) for t in td} == {(g, y) for g in GS for y in (False, True)}
    assert {(t["G"], t["q64"]) for t in td} == {(g, d) for g in GS for d in (False, True)}
    assert {t["rew64"] for t in td} == {False, True} and {t["done64"] for t in td} == {False, True} and {t["want_y"] for t in td} == {False, True}
    assert {(t["G"], b) for b, _, t in seen} >= {(8, BS.index(256)), (8, BS.index(257))}
    kinds = {(op, kind) for op, kind, _ in CONFIGS}
    assert kinds == {("td", "dqn"), ("td", "td3"), ("td", "sac"), ("al", "sac"), ("al", "tqc"), ("al", "td3"), ("al", "ent_coef")}
    assert {v.get("K") for op, kind, v in CONFIGS if op == "td" and kind != "dqn"} == {1, 2, 4}


# ================================================================================================= rsample, its backward, the smoothing
def _rs_members(G, B, dt, seed, start=5):
    """G members' actor outputs [B][2] (mean and log_std its two strided columns), each with its own seed and its own counter"""
    import torch
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    ms = []
    for i in range(G):
        ml = torch.randn(B, 2, dtype=dt, device="cuda", generator=g) * torch.tensor([0.8, 0.5], dtype=dt, device="cuda") + torch.tensor([0.0, -1.0], dtype=dt, device="cuda")
        ms.append(dict(ml=ml, mean=ml[:, :1], log_std=ml[:, 1:], counter=torch.full((1,), start + 3 * i, dtype=torch.int64, device="cuda"), seed=100 + i))
    return ms


def _rs_out(B, dt):
    import torch
    return (torch.full((B, 1), SENTINEL, dtype=dt, device="cuda"), torch.full((B, 1), SENTINEL, dtype=dt, device="cuda"),
            torch.full((B, 1), SENTINEL, dtype=torch.float64, device="cuda"))


@pytest.mark.parametrize("B", [1, 64, 65, 256, 257])
def test_rsample_its_backward_and_the_smoothing_bit_for_bit(B):
    import torch
    eng = _engine()
    for k, G in enumerate([1, 3, 8]):
        dt = _dt((B + k) % 2 == 1)
        a, b = _rs_members(G, B, dt, 7 * B + G), _rs_members(G, B, dt, 7 * B + G)
        starts = [int(m["counter"]) for m in a]
        assert len(set(starts)) == G
        pick = lambda m: {k_: m[k_] for k_ in ("mean", "log_std", "counter", "seed")}
        outs = [_rs_out(B, dt) for _ in range(G)]
        torch.cuda.synchronize()
        mem = _allocations()
        res = eng.rsample_group([dict(pick(m), out=o) for m, o in zip(a, outs)])
        assert _allocations() == mem
        singles = [eng.rsample(m["mean"], m["log_std"], m["counter"], seed=m["seed"], out=_rs_out(B, dt)) for m in b]
        eng.sync()
        for i, (r, s) in enumerate(zip(res, singles)):
            _same_results(r, s, f"rsample G={G} B={B} member {i}")
            assert bool(torch.isfinite(r.actions).all()) and not bool((r.noise == SENTINEL).any())
        assert [int(m["counter"]) for m in a] == [c + 1 for c in starts] == [int(m["counter"]) for m in b]          # every counter by exactly one
        assert G == 1 or not torch.equal(res[0].noise, res[1].noise)
        # deterministic: no counter is touched, the noise is zero
        det = eng.rsample_group([dict(pick(m), out=_rs_out(B, dt)) for m in a], deterministic=True)
        det1 = [eng.rsample(m["mean"], m["log_std"], m["counter"], seed=m["seed"], deterministic=True, out=_rs_out(B, dt)) for m in b]
        eng.sync()
        for i, (r, s) in enumerate(zip(det, det1)):
            _same_results(r, s, f"deterministic G={G} B={B} member {i}")
            assert not bool(r.noise.any())
        assert [int(m["counter"]) for m in a] == [c + 1 for c in starts]
        # the backward: only grad_actions, only grad_log_prob, both; the gradients land in the two strided columns of one [B][2] tensor
        g = torch.Generator(device="cuda"); g.manual_seed(B)
        ga = [torch.randn(B, 1, dtype=dt, device="cuda", generator=g) for _ in range(G)]
        gl = [torch.randn(B, 1, dtype=dt, device="cuda", generator=g) for _ in range(G)]
        for use_a, use_l in ((True, False), (False, True), (True, True)):
            cols = lambda: (lambda w: (w[:, :1], w[:, 1:]))(torch.full((B, 2), SENTINEL, dtype=dt, device="cuda"))
            back = eng.rsample_backward_group([dict(mean=m["mean"], log_std=m["log_std"], noise=r.noise, grad_actions=ga[i] if use_a else None,
                                                    grad_log_prob=gl[i] if use_l else None, out=cols()) for i, (m, r) in enumerate(zip(a, res))])
            back1 = [eng.rsample_backward(m["mean"], m["log_std"], s.noise, ga[i] if use_a else None, gl[i] if use_l else None, out=cols())
                     for i, (m, s) in enumerate(zip(b, singles))]
            eng.sync()
            for i, (r, s) in enumerate(zip(back, back1)):
                _same_results(r, s, f"backward {use_a} {use_l} G={G} B={B} member {i}")
                assert bool(torch.isfinite(r.grad_mean).all()) and bool(torch.isfinite(r.grad_log_std).all())
        # TD3's smoothing: every member its own noise_std, noise_clip and clip bounds
        sm = eng.smooth_target_action_group([dict(mean=m["mean"], counter=m["counter"], seed=m["seed"], clip=(-0.9 + 0.05 * i, 0.8 + 0.02 * i))
                                             for i, m in enumerate(a)], noise_std=[0.2 + 0.1 * i for i in range(G)], noise_clip=[0.5 + 0.05 * i for i in range(G)])
        sm1 = [eng.smooth_target_action(m["mean"], m["counter"], 0.2 + 0.1 * i, 0.5 + 0.05 * i, clip=(-0.9 + 0.05 * i, 0.8 + 0.02 * i), seed=m["seed"])
               for i, m in enumerate(b)]
        eng.sync()
        for i, (r, s) in enumerate(zip(sm, sm1)):
            _same(r, s, f"smoothing G={G} B={B} member {i}")
        assert [int(m["counter"]) for m in a] == [c + 2 for c in starts] == [int(m["counter"]) for m in b]


# ================================================================================================= a fault in member 1 of 3
@pytest.mark.parametrize("B", [65, 513])
def test_a_dqn_action_out_of_range_in_member_1_of_3(B):
    """PTG_E_INDEX once; the row's gradients stay as they were, and members 0 and 2 are what their own calls give"""
    import torch
    from rl_ptg_amd import _lib
    eng = _engine()

    def plant(ms):
        ms[1]["actions"][B // 2] = 5
    res, _ = _compare_loss(eng, 1, 3, B, seed=81, plant=plant, expect=_lib.E_INDEX)
    assert bool((res[1].grad_q[B // 2] == SENTINEL).all())    # never an address
    assert bool(torch.isnan(res[1].stats[0]))
    for i in (0, 2):
        assert bool(torch.isfinite(res[i].stats).all()) and bool(torch.isfinite(res[i].grad_q).all())


@pytest.mark.parametrize("B", [65, 513])
def test_a_nan_reward_in_member_1_of_3(B):
    import torch
    from rl_ptg_amd import _lib
    eng = _engine()

    def plant(ms):
        ms[1]["rewards"][B // 3] = float("nan")
    res, _ = _compare_loss(eng, 4, 3, B, seed=82, plant=plant, expect=_lib.E_NONFINITE)
    assert bool(torch.isnan(res[1].stats[0])) and all(bool(torch.isnan(g[B // 3])) for g in res[1].grad_q)
    for i in (0, 2):
        assert bool(torch.isfinite(res[i].stats).all()) and all(bool(torch.isfinite(g).all()) for g in res[i].grad_q)


@pytest.mark.parametrize("B", [65, 513])
def test_a_nan_log_prob_in_the_actor_loss_of_member_1_of_3(B):
    import torch
    from rl_ptg_amd import _lib
    eng = _engine()

    def plant(ms):
        ms[1]["log_prob"][B - 1] = float("nan")
    res, _ = _compare_loss(eng, 7, 3, B, seed=83, plant=plant, expect=_lib.E_NONFINITE)
    assert bool(torch.isnan(res[1].stats[0])) and bool(torch.isnan(res[1].grad_log_prob[B - 1])) and bool(torch.isnan(res[1].grad_log_ent_coef).all())
    for i in (0, 2):
        assert bool(torch.isfinite(res[i].stats).all()) and bool(torch.isfinite(res[i].grad_log_prob).all()) and bool(torch.isfinite(res[i].grad_log_ent_coef).all())


def test_a_nan_mean_in_rsample_of_member_1_of_3():
    import torch
    from rl_ptg_amd import _lib
    eng = _engine()
    B, dt = 65, torch.float32
    a, b = _rs_members(3, B, dt, 91), _rs_members(3, B, dt, 91)
    for ms in (a, b):
        ms[1]["ml"][7, 0] = float("nan")
    res = eng.rsample_group([dict(mean=m["mean"], log_std=m["log_std"], counter=m["counter"], seed=m["seed"], out=_rs_out(B, dt)) for m in a])
    _expect_error(eng, _lib.E_NONFINITE)
    singles = []
    for i, m in enumerate(b):
        singles.append(eng.rsample(m["mean"], m["log_std"], m["counter"], seed=m["seed"], out=_rs_out(B, dt)))
        if i == 1:
            _expect_error(eng, _lib.E_NONFINITE)
        else:
            eng.sync()
    for i, (r, s) in enumerate(zip(res, singles)):
        _same_results(r, s, f"member {i}")
    assert bool(torch.isnan(res[1].actions[7])) and int(torch.isnan(res[1].actions).sum()) == 1
    assert all(bool(torch.isfinite(res[i].actions).all()) and bool(torch.isfinite(res[i].log_prob).all()) for i in (0, 2))
    assert [int(m["counter"]) for m in a] == [6, 9, 12]


# ================================================================================================= smaller checks
def test_identical_bits_on_two_runs():
    eng = _engine()
    for c in (1, 5, 10):
        x, _ = _compare_loss(eng, c, 3, 513, seed=84)
        y, _ = _compare_loss(eng, c, 3, 513, seed=84)
        for r, s in zip(x, y):
            _same_results(r, s, f"two runs of {CONFIGS[c]}")


def test_no_host_synchronisation_no_allocation_and_nothing_else_touched():
    """A condition, not a timing (as tests/test_train_group.py checks its two ops): the stream is busy with milliseconds of fused steps
    before the grouped calls and still busy when they have returned, and they allocate no device memory.  Afterwards env state, vn
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
    B, dt = 513, torch.float32
    groups = []
    for c in (5, 7):
        op, kind, v = CONFIGS[c]
        made = [_member(eng, op, kind, v, i, B, False, True, False, False, True, 90 + c) for i in range(3)]
        groups.append((op, kind, [dict(m, out=o[0], workspace=o[1]) for m, o in ((m, o()) for m, o in made)]))
    rs = _rs_members(3, B, dt, 92)
    rs_out = [_rs_out(B, dt) for _ in rs]
    back_out = [(torch.empty(B, 1, device="cuda"), torch.empty(B, 1, device="cuda")) for _ in rs]
    ga = [torch.ones(B, 1, device="cuda") for _ in rs]

    def step():
        for op, kind, members in groups:
            eng.td_loss_group(kind, members) if op == "td" else eng.actor_loss_group(kind, members)
        res = eng.rsample_group([dict(mean=m["mean"], log_std=m["log_std"], counter=m["counter"], seed=m["seed"], out=o) for m, o in zip(rs, rs_out)])
        eng.rsample_backward_group([dict(mean=m["mean"], log_std=m["log_std"], noise=r.noise, grad_actions=a, grad_log_prob=None, out=o)
                                    for m, r, a, o in zip(rs, res, ga, back_out)])
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
    assert [int(m["counter"]) for m in rs] == [7, 10, 13]
    for _ in range(calls):
        twin.rollout(acts)
    twin.sync()
    a, b = eng.state_dict(), twin.state_dict()
    assert _equal_state(a["fields"], b["fields"]) and _equal_state(a["vn"], b["vn"])
    assert buf.cursor() == (0, 0)
    eng.close(); twin.close()


# ================================================================================================= the raw entries' refusals
def _copy(d, **kw):
    """a copy of a ctypes descriptor with fields replaced; `name[k]` addresses an array field"""
    c = type(d).from_buffer_copy(d)
    for k, v in kw.items():
        if "[" in k:
            name, idx = k[:-1].split("[")
            getattr(c, name)[int(idx)] = v
        else:
            setattr(c, k, v)
    return c


def _refusals(eng, entry, single, T, descs, bad, outputs, single_bad, single_text):
    """every (members, n, text) of `bad` through the raw grouped entry: PTG_E_INVALID, the text behind the entry's name, the stream idle,
    every output untouched; then the single entry's unchanged words, and the good group goes through"""
    import torch
    from rl_ptg_amd import _lib
    L, h, stream = eng._L, eng._h, eng._stream()
    arr = lambda ds: (T * max(len(ds), 1))(*ds)
    fn = getattr(L, entry)
    before = [t.clone() for t in outputs]
    torch.cuda.synchronize()
    for k, (ds, n, text) in enumerate(bad):
        assert fn(h, arr(ds), n, stream) == _lib.E_INVALID, (entry, k)
        err = L.ptg_last_error(h)
        assert err.startswith(entry.encode() + b": ") and text in err, (entry, k, err)
        assert torch.cuda.current_stream().query() is True, (entry, k)
    assert fn(h, None, 3, stream) == _lib.E_INVALID and b"null descriptor array" in L.ptg_last_error(h)
    assert fn(None, arr(descs), 3, stream) == _lib.E_INVALID
    for t, s in zip(outputs, before):
        _same(t, s, entry + ": an output of a refused call")
    assert getattr(L, single)(h, C.byref(single_bad), stream) == _lib.E_INVALID
    assert L.ptg_last_error(h) == single_text
    assert fn(h, arr(descs), len(descs), stream) == 0, L.ptg_last_error(h)
    eng.sync()


def test_c_level_refusals_of_the_two_losses_enqueue_nothing():
    import torch
    from rl_ptg_amd import _lib
    eng = _engine()
    B = 65
    # ---- td: three SAC members with log alpha (flags 3), K = 2, the target written
    made = [_member(eng, "td", "sac", dict(K=2, alpha="log"), i, B, False, True, False, False, True, 95) for i in range(3)]
    outs = [o() for _, o in made]
    td = [eng._td_loss_member("t", "sac", **dict(m, out=o, workspace=w))[1]()[0] for (m, _), (o, w) in zip(made, outs)]
    d3 = lambda **kw: [td[0], td[1], _copy(td[2], **kw)]
    dqn = [_member(eng, "td", "dqn", dict(A=5, act="i64"), i, B, False, False, False, False, False, 96) for i in range(3)]
    dq = [eng._td_loss_member("t", "dqn", **dict(m, out=o, workspace=w))[1]()[0] for (m, _), (o, w) in zip(dqn, [o() for _, o in dqn])]
    q3 = lambda **kw: [dq[0], dq[1], _copy(dq[2], **kw)]
    bad = [
        (td, 0, b"n_members 0 outside"), (td * 3, 9, b"n_members 9 outside"), (td, -1, b"n_members -1 outside"),
        (d3(batch=0), 3, b"member 2: batch 0 outside [1, 2^31]"), (d3(rew_dev=None), 3, b"member 2: null rew_dev, done_dev or stats_dev"),
        ([td[0], _copy(td[1], kind=7), td[2]], 3, b"member 1: unknown kind 7"), (d3(ws_dev=None), 3, b"member 2: ws_dev is null"),
        (d3(**{"q_dev[1]": None}), 3, b"member 2: null q_dev, next_q_dev or grad_q_dev [1]"), (d3(alpha_dev=None), 3, b"member 2: PTG_TD_LOG_ALPHA needs alpha_dev"),
        (q3(kind=_lib.TD_CRITICS, n_critics=1), 3, b"members 0 and 2 disagree in kind: 0 and 1"), (d3(flags=_lib.TD_ENTROPY), 3, b"members 0 and 2 disagree in flags: 3 and 1"),
        (q3(n_actions=4), 3, b"members 0 and 2 disagree in n_actions: 5 and 4"), (d3(n_critics=1), 3, b"members 0 and 2 disagree in n_critics: 2 and 1"),
        (d3(q_dtype=_lib.OUT_F64), 3, b"members 0 and 2 disagree in q_dtype"), (d3(rew_dtype=_lib.OUT_F64), 3, b"members 0 and 2 disagree in rew_dtype"),
        (d3(done_dtype=_lib.OUT_F64), 3, b"members 0 and 2 disagree in done_dtype"), (q3(act_kind=_lib.ACT_I32), 3, b"members 0 and 2 disagree in act_kind"),
        (d3(batch=64), 3, b"members 0 and 2 disagree in batch: 65 and 64"),
        (d3(stats_dev=td[0].stats_dev), 3, b"members 0 and 2 share stats_dev"), (d3(ws_dev=td[1].ws_dev), 3, b"members 1 and 2 share ws_dev"),
        (d3(y_dev=td[0].y_dev), 3, b"members 0 and 2 share y_dev"), (d3(**{"grad_q_dev[0]": td[1].grad_q_dev[1]}), 3, b"members 1 and 2 share grad_q_dev"),
    ]
    flat = [t for o, w in outs for _, t in _flat(o)] + [w for _, w in outs]
    _refusals(eng, "ptg_td_loss_group", "ptg_td_loss", _lib.PtgTd, td, bad, flat, _copy(td[0], batch=0), b"ptg_td_loss: batch 0 outside [1, 2^31]")
    # ---- the actor loss: three SAC members with log alpha and the entropy-coefficient loss (flags 7), K = 2
    made = [_member(eng, "al", "sac", dict(K=2, alpha="log", ec=True), i, B, False, True, False, False, False, 97) for i in range(3)]
    outs = [o() for _, o in made]
    al = [eng._actor_loss_member("t", "sac", **dict(m, out=o, workspace=w))[1]()[0] for (m, _), (o, w) in zip(made, outs)]
    a3 = lambda **kw: [al[0], al[1], _copy(al[2], **kw)]
    tq = [_member(eng, "al", "tqc", dict(K=2, Q=25, alpha="mixed"), i, B, False, False, False, False, False, 98) for i in range(3)]
    tqd = [eng._actor_loss_member("t", "tqc", **dict(m, out=o, workspace=w))[1]()[0] for (m, _), (o, w) in zip(tq, [o() for _, o in tq])]
    bad = [
        (al, 0, b"n_members 0 outside"), (al * 3, 9, b"n_members 9 outside"), (al, -1, b"n_members -1 outside"),
        (a3(batch=0), 3, b"member 2: batch 0 outside"), (a3(stats_dev=None), 3, b"member 2: null stats_dev"),
        ([al[0], _copy(al[1], logp_dev=None), al[2]], 3, b"member 1: PTG_AL_ENTROPY and PTG_AL_ENT_COEF need logp_dev"),
        (a3(target_entropy=float("inf")), 3, b"member 2: PTG_AL_ENT_COEF needs a finite target_entropy"),
        (a3(kind=_lib.AL_MEAN, n_quantiles=1), 3, b"members 0 and 2 disagree in kind: 0 and 1"),
        (a3(flags=_lib.AL_ENTROPY | _lib.AL_LOG_ALPHA, grad_log_alpha_dev=None), 3, b"members 0 and 2 disagree in flags: 7 and 3"),
        (a3(n_critics=1), 3, b"members 0 and 2 disagree in n_critics: 2 and 1"), ([tqd[0], tqd[1], _copy(tqd[2], n_quantiles=24)], 3, b"members 0 and 2 disagree in n_quantiles: 25 and 24"),
        (a3(q_dtype=_lib.OUT_F64), 3, b"members 0 and 2 disagree in q_dtype"), (a3(batch=64), 3, b"members 0 and 2 disagree in batch: 65 and 64"),
        (a3(stats_dev=al[1].stats_dev), 3, b"members 1 and 2 share stats_dev"), (a3(ws_dev=al[0].ws_dev), 3, b"members 0 and 2 share ws_dev"),
        (a3(**{"grad_q_dev[1]": al[0].grad_q_dev[0]}), 3, b"members 0 and 2 share grad_q_dev"), (a3(grad_logp_dev=al[0].grad_logp_dev), 3, b"members 0 and 2 share grad_logp_dev"),
        (a3(grad_log_alpha_dev=al[1].grad_log_alpha_dev), 3, b"members 1 and 2 share grad_log_alpha_dev"),
    ]
    flat = [t for o, w in outs for _, t in _flat(o)] + [w for _, w in outs]
    _refusals(eng, "ptg_actor_loss_group", "ptg_actor_loss", _lib.PtgAl, al, bad, flat, _copy(al[0], batch=0), b"ptg_actor_loss: batch 0 outside [1, 2^31]")


def test_c_level_refusals_of_rsample_and_its_backward_enqueue_nothing():
    import torch
    from rl_ptg_amd import _lib
    eng = _engine()
    B, dt = 65, torch.float32
    ms = _rs_members(3, B, dt, 99)
    outs = [_rs_out(B, dt) for _ in ms]
    rs = [eng._rsample_member("t", m["mean"], m["log_std"], m["counter"], seed=m["seed"], out=o)[1]()[0] for m, o in zip(ms, outs)]
    r3 = lambda **kw: [rs[0], rs[1], _copy(rs[2], **kw)]
    bad = [
        (rs, 0, b"n_members 0 outside"), (rs * 3, 9, b"n_members 9 outside"), (rs, -1, b"n_members -1 outside"),
        (r3(batch=0), 3, b"member 2: batch outside [1, 2^31]"), (r3(mean_dev=None), 3, b"member 2: null mean_dev or mean_s_n < 1"),
        ([rs[0], _copy(rs[1], counter_dev=None), rs[2]], 3, b"member 1: a stochastic call needs counter_dev"),
        (r3(kind=_lib.RS_SMOOTH, logp_dev=None), 3, b"members 0 and 2 disagree in kind: 0 and 1"), (r3(flags=_lib.RS_DETERMINISTIC), 3, b"members 0 and 2 disagree in flags: 0 and 1"),
        (r3(q_dtype=_lib.OUT_F64), 3, b"members 0 and 2 disagree in q_dtype"), (r3(batch=64), 3, b"members 0 and 2 disagree in batch: 65 and 64"),
        (r3(act_dev=rs[0].act_dev), 3, b"members 0 and 2 share act_dev"), (r3(logp_dev=rs[1].logp_dev), 3, b"members 1 and 2 share logp_dev"),
        (r3(noise_dev=rs[0].noise_dev), 3, b"members 0 and 2 share noise_dev"), (r3(counter_dev=rs[1].counter_dev), 3, b"members 1 and 2 share counter_dev"),
    ]
    counters = [m["counter"] for m in ms]
    _refusals(eng, "ptg_rsample_group", "ptg_rsample", _lib.PtgRs, rs, bad, [t for o in outs for t in o] + counters, _copy(rs[0], batch=0),
              b"ptg_rsample: batch outside [1, 2^31]")
    assert [int(c) for c in counters] == [6, 9, 12]          # the one accepted call
    # deterministic members may share a counter pointer: it is not read
    det = [_copy(d, flags=_lib.RS_DETERMINISTIC, counter_dev=rs[0].counter_dev) for d in rs]
    assert eng._L.ptg_rsample_group(eng._h, (_lib.PtgRs * 3)(*det), 3, eng._stream()) == 0, eng._L.ptg_last_error(eng._h)
    eng.sync()
    assert [int(c) for c in counters] == [6, 9, 12]
    # ---- the backward
    ga = [torch.ones(B, 1, device="cuda") for _ in ms]
    gouts = [(torch.full((B, 1), SENTINEL, device="cuda"), torch.full((B, 1), SENTINEL, device="cuda")) for _ in ms]
    bw = [eng._rsample_backward_member("t", m["mean"], m["log_std"], o[2], a, None, out=g)[1]()[0] for m, o, a, g in zip(ms, outs, ga, gouts)]
    b3 = lambda **kw: [bw[0], bw[1], _copy(bw[2], **kw)]
    bad = [
        (bw, 0, b"n_members 0 outside"), (bw * 3, 9, b"n_members 9 outside"), (bw, -1, b"n_members -1 outside"),
        (b3(noise_dev=None), 3, b"member 2: noise_dev is null or not aligned to 8 bytes"), (b3(grad_act_dev=None), 3, b"member 2: grad_act_dev and grad_logp_dev are both null"),
        ([bw[0], _copy(bw[1], kind=_lib.RS_SMOOTH), bw[2]], 3, b"member 1: PTG_RS_SMOOTH has no backward"),
        (b3(q_dtype=_lib.OUT_F64), 3, b"members 0 and 2 disagree in q_dtype"), (b3(batch=64), 3, b"members 0 and 2 disagree in batch: 65 and 64"),
        (b3(flags=_lib.RS_DETERMINISTIC), 3, b"members 0 and 2 disagree in flags"),
        (b3(grad_mean_dev=bw[0].grad_log_std_dev), 3, b"members 0 and 2 share grad_mean_dev and grad_log_std_dev"),
        (b3(grad_log_std_dev=bw[1].grad_mean_dev), 3, b"members 1 and 2 share grad_mean_dev and grad_log_std_dev"),
        (b3(grad_mean_dev=bw[0].grad_mean_dev), 3, b"members 0 and 2 share grad_mean_dev"), (b3(grad_log_std_dev=bw[1].grad_log_std_dev), 3, b"members 1 and 2 share grad_log_std_dev"),
    ]
    _refusals(eng, "ptg_rsample_backward_group", "ptg_rsample_backward", _lib.PtgRs, bw, bad, [t for g in gouts for t in g], _copy(bw[0], noise_dev=None),
              b"ptg_rsample_backward: noise_dev is null or not aligned to 8 bytes")


# ================================================================================================= together
F, H = 40, 32


def _mlp(seed, fan_in, out, tanh_out=False):
    import torch
    from torch import nn
    torch.manual_seed(seed)
    layers = [nn.Linear(fan_in, H), nn.Tanh(), nn.Linear(H, out)] + ([nn.Tanh()] if tanh_out else [])
    return nn.Sequential(*layers).cuda()


def _params(mods):
    return [p for m in mods for p in m.parameters()]


def _optimizer(eng, params, **kw):
    import torch
    from rl_ptg_amd import DeviceOptimizer
    for p in params:
        p.grad = torch.zeros_like(p)
    return DeviceOptimizer(eng, params, kind="adam", zero_grad=True, **kw)


def _set_grads(params, grads):
    for p, g in zip(params, grads):
        p.grad.copy_(g)


def _opt_state(o):
    p = o.plan
    return p.state1 + p.state2 + [p.state]


def _batches(G, B, steps, seed, discrete=0):
    import torch
    gen = torch.Generator(device="cuda"); gen.manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=gen)
    one = lambda: dict(obs=rn(B, F), next_obs=rn(B, F), actions=torch.randint(0, discrete, (B,), device="cuda", generator=gen) if discrete else rn(B, 1).tanh(),
                       rewards=rn(B), dones=(torch.rand(B, device="cuda", generator=gen) < 0.2).float())
    return [[one() for _ in range(G)] for _ in range(steps)]


@pytest.mark.parametrize("G,B", [(3, 21), (2, 300)], ids=["three-agents-one-launch", "two-agents-rows-plus-final"])
def test_sac_agents_eager_captured_and_replayed_against_single_twins(G, B):
    """B = 300 is the two-launch path of every loss (rows + final merge over each member's own workspace, which the front ends allocate:
    no workspace= anywhere) inside the captured graph.  Three SAC agents, B = 21: the three actors (40 -> 32 -> 2) in one TrainMLPGroup, the six critics (40 + 1 -> 32 -> 1, the two-piece
    input) in one, the six targets in one DeviceMLPGroup, the actors', critics' and log alphas' optimisers in three DeviceOptimizerGroups;
    SB3's SAC.train through the *_group functions.  One eager step, a capture on a side stream (at the default hardware-queue setting),
    three replays with the batch tensors rewritten in place.  After every step every parameter, Adam state, target and log alpha of every
    agent equals, bit for bit, a twin agent's that steps singly: TrainMLP, TrainMLPGroup of its two critics, squashed_rsample,
    ent_coef_loss, sac_critic_loss, sac_actor_loss, DeviceOptimizer."""
    import torch
    from rl_ptg_amd import (DeviceMLPGroup, DeviceOptimizerGroup, TrainMLP, TrainMLPGroup, ent_coef_loss, ent_coef_loss_group, sac_actor_loss, sac_actor_loss_group,
                            sac_critic_loss, sac_critic_loss_group, squashed_rsample, squashed_rsample_group)
    eng = _engine(6)
    gamma, lr, tau, H_t, la0, seeds = ([0.96, 0.97, 0.98][:G], [3e-3, 1e-3, 2e-3][:G], [0.005, 0.01, 0.02][:G], [-1.0, -0.8, -1.2][:G], [-1.0, -0.5, -1.5][:G],
                                       [21, 22, 23][:G])
    steps = _batches(G, B, 4, 5)

    class Agent:
        def __init__(self, i):
            self.i = i
            self.actor = _mlp(50 + i, F, 2)
            with torch.no_grad():
                self.actor[2].weight.mul_(0.3); self.actor[2].bias[1] = -1.0
            self.critics = [_mlp(60 + 2 * i + k, F + 1, 1) for k in range(2)]
            self.targets = [_mlp(60 + 2 * i + k, F + 1, 1) for k in range(2)]
            self.log_alpha = torch.tensor([la0[i]], dtype=torch.float64, device="cuda", requires_grad=True)
            self.counter = torch.full((1,), 3 + i, dtype=torch.int64, device="cuda")
            self.ap, self.cp, self.tp = _params([self.actor]), _params(self.critics), _params(self.targets)
            self.opt_a = _optimizer(eng, self.ap, lr=lr[i])
            self.opt_c = _optimizer(eng, self.cp, lr=lr[i], targets=self.tp, tau=tau[i])
            self.opt_l = _optimizer(eng, [self.log_alpha], lr=10 * lr[i])

        def everything(self):
            return self.ap + self.cp + self.tp + [self.log_alpha] + _opt_state(self.opt_a) + _opt_state(self.opt_c) + _opt_state(self.opt_l) + [self.counter]

    agents, twins = [Agent(i) for i in range(G)], [Agent(i) for i in range(G)]
    static = [{k: v.clone() for k, v in b.items()} for b in steps[0]]
    actors = TrainMLPGroup(eng, [a.actor for a in agents], batch=B)
    actors_nograd = DeviceMLPGroup(eng, [a.actor for a in agents], batch=B)
    critics = TrainMLPGroup(eng, [m for a in agents for m in a.critics], batch=B)
    targets = DeviceMLPGroup(eng, [m for a in agents for m in a.targets], batch=B)
    og_a, og_c, og_l = (DeviceOptimizerGroup(eng, [getattr(a, n) for a in agents]) for n in ("opt_a", "opt_c", "opt_l"))
    twice = lambda xs: [x for x in xs for _ in range(2)]

    def grouped_step():
        s = static
        ml = actors([b["obs"] for b in s])
        pi = squashed_rsample_group(eng, [dict(mean=o[:, :1], log_std=o[:, 1:], counter=a.counter) for o, a in zip(ml, agents)], seed=seeds)
        els, el_stats = ent_coef_loss_group(eng, [dict(log_prob=lp, log_ent_coef=a.log_alpha) for (_, lp), a in zip(pi, agents)], target_entropy=H_t)
        alphas = [st[4:5] for st in el_stats]                # the alpha from before the alpha step, on the device
        torch.autograd.backward(els)
        og_l.step()
        with torch.no_grad():
            nml = actors_nograd([b["next_obs"] for b in s])
            nxt = squashed_rsample_group(eng, [dict(mean=o[:, :1], log_std=o[:, 1:], counter=a.counter) for o, a in zip(nml, agents)], seed=seeds)
            nq = targets(twice([b["next_obs"] for b in s]), x2=twice([na for na, _ in nxt]))
        q = critics(twice([b["obs"] for b in s]), x2=twice([b["actions"] for b in s]))
        closses, _ = sac_critic_loss_group(eng, [dict(q=list(q[2 * i:2 * i + 2]), next_q=list(nq[2 * i:2 * i + 2]), rewards=s[i]["rewards"], dones=s[i]["dones"],
                                                      next_log_prob=nxt[i][1], ent_coef=alphas[i]) for i in range(G)], gamma=gamma)
        torch.autograd.backward(closses)
        og_c.step()
        q_pi = critics(twice([b["obs"] for b in s]), x2=twice([a_pi for a_pi, _ in pi]))
        alosses, _ = sac_actor_loss_group(eng, [dict(q=list(q_pi[2 * i:2 * i + 2]), log_prob=pi[i][1], ent_coef=alphas[i]) for i in range(G)])
        all_ap = [p for a in agents for p in a.ap]
        _set_grads(all_ap, torch.autograd.grad(alosses, all_ap))     # the actors' parameters alone, as SB3's actor optimiser sees them
        og_a.step()

    class Twin:
        def __init__(self, a):
            self.a = a
            self.actor, self.actor_nograd = TrainMLP(eng, a.actor, batch=B), DeviceMLPGroup(eng, [a.actor], batch=B)
            self.critics, self.targets = TrainMLPGroup(eng, a.critics, batch=B), DeviceMLPGroup(eng, a.targets, batch=B)

        def __call__(self, b):
            a, i = self.a, self.a.i
            ml = self.actor(b["obs"])
            a_pi, lp = squashed_rsample(eng, ml[:, :1], ml[:, 1:], a.counter, seed=seeds[i])
            el, el_stats = ent_coef_loss(eng, lp, a.log_alpha, target_entropy=H_t[i])
            alpha = el_stats[4:5]
            el.backward()
            a.opt_l.step()
            with torch.no_grad():
                nml, = self.actor_nograd(b["next_obs"])
                na, nlp = squashed_rsample(eng, nml[:, :1], nml[:, 1:], a.counter, seed=seeds[i])
                nq = self.targets(b["next_obs"], x2=na)
            q = self.critics(b["obs"], x2=b["actions"])
            cl, _ = sac_critic_loss(eng, list(q), list(nq), b["rewards"], b["dones"], nlp, gamma=gamma[i], ent_coef=alpha)
            cl.backward()
            a.opt_c.step()
            q_pi = self.critics(b["obs"], x2=a_pi)
            al, _ = sac_actor_loss(eng, list(q_pi), lp, ent_coef=alpha)
            _set_grads(a.ap, torch.autograd.grad(al, a.ap))
            a.opt_a.step()
    singles = [Twin(t) for t in twins]

    def check(step):
        torch.cuda.synchronize()
        eng.sync()
        for i, (a, t) in enumerate(zip(agents, twins)):
            for k, (x, y) in enumerate(zip(a.everything(), t.everything())):
                _same(x, y, f"step {step} agent {i} tensor {k}")
            assert int(a.counter) == 3 + i + 2 * (step + 1)
    start = [p.detach().clone() for a in agents for p in a.ap + a.cp + a.tp + [a.log_alpha]]
    grouped_step()                                           # the eager step
    for t, b in zip(singles, steps[0]):
        t(b)
    check(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            grouped_step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert float(agents[0].opt_c.plan.state[0]) == 1.0 and int(agents[0].counter) == 5       # capturing ran nothing
    for step in range(1, 4):
        for i in range(G):
            for k, v in steps[step][i].items():
                static[i][k].copy_(v)
        graph.replay()
        for t, b in zip(singles, steps[step]):
            t(b)
        check(step)
    now = [p.detach() for a in agents for p in a.ap + a.cp + a.tp + [a.log_alpha]]
    assert all(not torch.equal(x, y) and bool(torch.isfinite(y).all()) for x, y in zip(start, now))
    assert [float(a.opt_a.plan.state[0]) for a in agents] == [4.0] * G


def test_two_td3_agents_with_smoothing_and_a_delayed_actor_against_single_twins():
    """Two TD3 agents, B = 21, two eager gradient steps under policy_delay = 2: the first also steps the actors, the second does not"""
    import torch
    from rl_ptg_amd import DeviceMLPGroup, DeviceOptimizerGroup, TrainMLP, TrainMLPGroup, td3_actor_loss, td3_actor_loss_group, td3_critic_loss, td3_critic_loss_group
    eng = _engine(6)
    G, B = 2, 21
    gamma, lr, tau, sd, nc, seeds = [0.98, 0.97], [1e-3, 2e-3], [0.005, 0.02], [0.2, 0.3], [0.5, 0.4], [31, 32]
    steps = _batches(G, B, 2, 6)

    class Agent:
        def __init__(self, i):
            self.i = i
            self.actor, self.actor_t = _mlp(70 + i, F, 1, True), _mlp(70 + i, F, 1, True)
            self.critics = [_mlp(80 + 2 * i + k, F + 1, 1) for k in range(2)]
            self.targets = [_mlp(80 + 2 * i + k, F + 1, 1) for k in range(2)]
            self.counter = torch.full((1,), 11 + i, dtype=torch.int64, device="cuda")
            self.ap, self.cp = _params([self.actor]), _params(self.critics)
            self.opt_a = _optimizer(eng, self.ap, lr=lr[i], targets=_params([self.actor_t]), tau=tau[i])
            self.opt_c = _optimizer(eng, self.cp, lr=lr[i], targets=_params(self.targets), tau=tau[i])

        def everything(self):
            return self.ap + self.cp + _params([self.actor_t]) + _params(self.targets) + _opt_state(self.opt_a) + _opt_state(self.opt_c) + [self.counter]

    agents, twins = [Agent(i) for i in range(G)], [Agent(i) for i in range(G)]
    actors = TrainMLPGroup(eng, [a.actor for a in agents], batch=B)
    actor_ts = DeviceMLPGroup(eng, [a.actor_t for a in agents], batch=B)
    critics = TrainMLPGroup(eng, [m for a in agents for m in a.critics], batch=B)
    targets = DeviceMLPGroup(eng, [m for a in agents for m in a.targets], batch=B)
    og_a, og_c = (DeviceOptimizerGroup(eng, [getattr(a, n) for a in agents]) for n in ("opt_a", "opt_c"))
    twice = lambda xs: [x for x in xs for _ in range(2)]

    def grouped_step(s, with_actor):
        with torch.no_grad():
            means = actor_ts([b["next_obs"] for b in s])
            na = eng.smooth_target_action_group([dict(mean=m, counter=a.counter) for m, a in zip(means, agents)], noise_std=sd, noise_clip=nc, seed=seeds)
            nq = targets(twice([b["next_obs"] for b in s]), x2=twice(na))
        q = critics(twice([b["obs"] for b in s]), x2=twice([b["actions"] for b in s]))
        closses, _ = td3_critic_loss_group(eng, [dict(q=list(q[2 * i:2 * i + 2]), next_q=list(nq[2 * i:2 * i + 2]), rewards=s[i]["rewards"], dones=s[i]["dones"])
                                                 for i in range(G)], gamma=gamma)
        torch.autograd.backward(closses)
        og_c.step()
        if with_actor:
            acts = actors([b["obs"] for b in s])
            q_pi = critics(twice([b["obs"] for b in s]), x2=twice(acts))
            alosses, _ = td3_actor_loss_group(eng, [dict(q1=q_pi[2 * i]) for i in range(G)])
            all_ap = [p for a in agents for p in a.ap]
            _set_grads(all_ap, torch.autograd.grad(alosses, all_ap))
            og_a.step()

    def single_step(a, b, with_actor, nets):
        actor, actor_t, crit, targ = nets
        i = a.i
        with torch.no_grad():
            mean, = actor_t(b["next_obs"])
            na = eng.smooth_target_action(mean, a.counter, sd[i], nc[i], seed=seeds[i])
            nq = targ(b["next_obs"], x2=na)
        q = crit(b["obs"], x2=b["actions"])
        cl, _ = td3_critic_loss(eng, list(q), list(nq), b["rewards"], b["dones"], gamma=gamma[i])
        cl.backward()
        a.opt_c.step()
        if with_actor:
            q_pi = crit(b["obs"], x2=actor(b["obs"]))
            al, _ = td3_actor_loss(eng, q_pi[0])
            _set_grads(a.ap, torch.autograd.grad(al, a.ap))
            a.opt_a.step()
    nets = [(TrainMLP(eng, t.actor, batch=B), DeviceMLPGroup(eng, [t.actor_t], batch=B), TrainMLPGroup(eng, t.critics, batch=B), DeviceMLPGroup(eng, t.targets, batch=B))
            for t in twins]
    start = [p.detach().clone() for a in agents for p in a.ap + a.cp]
    for step in range(2):
        grouped_step(steps[step], step % 2 == 0)
        for t, b, n in zip(twins, steps[step], nets):
            single_step(t, b, step % 2 == 0, n)
        torch.cuda.synchronize()
        eng.sync()
        for i, (a, t) in enumerate(zip(agents, twins)):
            for k, (x, y) in enumerate(zip(a.everything(), t.everything())):
                _same(x, y, f"step {step} agent {i} tensor {k}")
    assert all(not torch.equal(x, y.detach()) for x, y in zip(start, [p for a in agents for p in a.ap + a.cp]))
    assert [float(a.opt_a.plan.state[0]) for a in agents] == [1.0] * G and [float(a.opt_c.plan.state[0]) for a in agents] == [2.0] * G


def test_two_dqn_agents_with_a_hard_target_update_against_single_twins():
    """Two DQN agents, B = 21, one eager step; the hard target update is the optimiser group's Polyak with tau = 1"""
    import torch
    from rl_ptg_amd import DeviceMLPGroup, DeviceOptimizerGroup, TrainMLP, TrainMLPGroup, dqn_loss, dqn_loss_group
    eng = _engine(6)
    G, B, A = 2, 21, 5
    gamma, lr = [0.99, 0.95], [1e-3, 3e-3]
    batch = _batches(G, B, 1, 7, discrete=A)[0]

    class Agent:
        def __init__(self, i):
            self.q, self.q_t = _mlp(90 + i, F, A), _mlp(95 + i, F, A)
            self.qp, self.tp = _params([self.q]), _params([self.q_t])
            self.opt = _optimizer(eng, self.qp, lr=lr[i], max_grad_norm=10.0, targets=self.tp, tau=1.0)

    agents, twins = [Agent(i) for i in range(G)], [Agent(i) for i in range(G)]
    q = TrainMLPGroup(eng, [a.q for a in agents], batch=B)([b["obs"] for b in batch])
    with torch.no_grad():
        nq = DeviceMLPGroup(eng, [a.q_t for a in agents], batch=B)([b["next_obs"] for b in batch])
    losses, stats = dqn_loss_group(eng, [dict(q=q[i], next_q=nq[i], actions=b["actions"], rewards=b["rewards"], dones=b["dones"]) for i, b in enumerate(batch)], gamma=gamma)
    torch.autograd.backward(losses)
    DeviceOptimizerGroup(eng, [a.opt for a in agents]).step()
    for i, (t, b) in enumerate(zip(twins, batch)):
        with torch.no_grad():
            nq1, = DeviceMLPGroup(eng, [t.q_t], batch=B)(b["next_obs"])
        loss, st = dqn_loss(eng, TrainMLP(eng, t.q, batch=B)(b["obs"]), nq1, b["actions"], b["rewards"], b["dones"], gamma=gamma[i])
        loss.backward()
        t.opt.step()
        _same(losses[i], loss, f"agent {i} loss")
        _same(stats[i], st, f"agent {i} stats")
    torch.cuda.synchronize()
    eng.sync()
    for i, (a, t) in enumerate(zip(agents, twins)):
        for k, (x, y) in enumerate(zip(a.qp + a.tp + _opt_state(a.opt) + [a.opt.plan.norm], t.qp + t.tp + _opt_state(t.opt) + [t.opt.plan.norm])):
            _same(x, y, f"agent {i} tensor {k}")
        for p, tp in zip(a.qp, a.tp):
            _same(p, tp, f"agent {i}: tau = 1 is a copy")
