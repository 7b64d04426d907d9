"""What the gSDE ops (ptg_sde_resample, ptg_sde_act, ptg_sde_policy_loss) rest on that needs no GPU: tests/sde_restatement.py against
SB3's own expressions under torch float64 autograd (the loss and all four gradients within 1e-10 relative), its shared lines against
tests/policy_loss_restatement.py bit for bit, a 2-row case by hand, sample()'s identity, the layout of the RNG keys, the three
descriptors as gcc sees them, the workspace size against its Python restatement and every Python-level refusal with nothing touched."""
import ctypes as C
import os

import numpy as np
import pytest

import act_restatement as ar
import policy_loss_restatement as plr
import sde_restatement as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.max(np.abs(np.asarray(got, np.float64) - ref) / np.maximum(np.abs(ref).max(), 1e-300)))


@pytest.mark.parametrize("kind,norm,cvf", sr.CONFIGS)
@pytest.mark.parametrize("B,L", [(1, 1), (2, 2), (5, 65), (203, 358), (257, 129)])
def test_the_restatement_against_sb3s_expressions_under_autograd(kind, norm, cvf, B, L):
    c = sr.loss_case(B, L, np.float64)
    kw = sr.loss_kwargs(kind, norm, cvf)
    r = sr.policy_loss(kind, c["mean"], c["values"], c["latent"], c["log_std"], c["actions"], c["old_log_prob"], c["advantages"], c["returns"],
                       old_values=c["old_values"], **kw)
    t = sr.torch_reference(kind, c, clip_range_vf=cvf, normalize_advantage=norm)
    assert not r["bad"].any()
    worst = {"loss": abs(r["stats"][0] - t["stats"][0]) / max(abs(t["stats"][0]), 1e-300)}
    for k in ("grad_input", "grad_values", "grad_log_std", "grad_latent"):
        worst[k] = _rel(r[k], t[k]) if np.abs(t[k]).max() > 0 else float(np.abs(r[k]).max())
    for k in range(1, 6):
        assert abs(r["stats"][k] - t["stats"][k]) <= 1e-10 * max(1.0, abs(t["stats"][k])), (k, r["stats"], t["stats"])
    assert max(worst.values()) <= 1e-10, worst


@pytest.mark.parametrize("kind,norm,cvf", sr.CONFIGS)
def test_the_shared_lines_are_policy_loss_restatements_bit_for_bit(kind, norm, cvf):
    """lines() fed with the log-probabilities and entropies of that module's Gaussian head returns that module's statistics, value
    gradients and -- through grad_input = ((-g) * (z / sigma)) / B -- its g"""
    for B in (1, 2, 203, 257):
        c = plr.gaussian_case(B, np.float64)
        kw = sr.loss_kwargs(kind, norm, cvf)
        ref = plr.policy_loss(kind, c["mean"], c["values"], c["actions"], c["old_log_prob"], c["advantages"], c["returns"], old_values=c["old_values"],
                              log_std=c["log_std"], **kw)
        ls = float(c["log_std"][0])
        lp = plr.log_prob(c["mean"], c["actions"], c["log_std"])
        got = sr.lines(kind, lp, np.full(B, 1.4189385332046727 + ls), np.zeros(B, bool), c["values"], c["old_log_prob"], c["advantages"], c["returns"],
                       old_values=c["old_values"], **kw)
        assert np.array_equal(got["stats"], ref["stats"]) and np.array_equal(got["grad_values"], ref["grad_values"])
        z = (c["actions"] - c["mean"]) / np.exp(ls)
        assert np.array_equal(((-got["g"]) * (z / np.exp(ls))) / float(B), ref["grad_input"])
        assert got["abs_mean"] == ref["abs_mean"] and got["margin"] == ref["margin"]


def test_two_rows_by_hand():
    """L = 2, log_std = log([2, 1/2]) so s^2 = [4, 1/4]; rows h = [1, 2] and [0, 4]; A2C without normalisation, c_e = 0, c_v = 1"""
    ls = np.log(np.array([2.0, 0.5]))
    h = np.array([[1.0, 2.0], [0.0, 4.0]])
    mu, a = np.array([0.5, -1.0]), np.array([1.5, 1.0])
    adv, ret, val = np.array([2.0, -1.0]), np.array([1.0, 0.0]), np.array([0.0, 3.0])
    r = sr.policy_loss("a2c", mu, val, h, ls, a, None, adv, ret, ent_coef=0.0, vf_coef=1.0, normalize_advantage=False)
    V = np.array([1 * 4 + 4 * 0.25 + 1e-6, 16 * 0.25 + 1e-6])                     # 5 and 4, plus epsilon
    np.testing.assert_allclose(r["V"], V, rtol=1e-15)
    d = a - mu                                                                   # 1 and 2
    lp = -d * d / (2 * V) - 0.5 * np.log(V) - 0.5 * np.log(2 * np.pi)
    np.testing.assert_allclose(r["stats"][1], -(adv * lp).mean(), rtol=1e-14)
    np.testing.assert_allclose(r["stats"][2], ((ret - val) ** 2).mean(), rtol=1e-15)   # (1 + 9) / 2
    np.testing.assert_allclose(r["stats"][3], -(0.5 + 0.5 * np.log(2 * np.pi) + 0.5 * np.log(V)).mean(), rtol=1e-14)
    np.testing.assert_allclose(r["grad_input"], -adv * d / V / 2, rtol=1e-14)        # [-0.2, 0.25] up to epsilon
    np.testing.assert_allclose(r["grad_values"], [2 * (0.0 - 1.0) / 2, 2 * (3.0 - 0.0) / 2], rtol=1e-15)
    c = -adv * (d * d / V - 1) / (2 * V)                                         # row 0: -2 * (1/5 - 1) / 10 = 0.16; row 1: 1 * (1 - 1) / 8 = 0
    np.testing.assert_allclose(c, [0.16, 0.0], atol=1e-6)
    np.testing.assert_allclose(r["grad_log_std"], 2 * np.array([4.0, 0.25]) * (c[:, None] * h * h).sum(0) / 2, rtol=1e-13, atol=1e-18)
    np.testing.assert_allclose(r["grad_latent"], c[:, None] * 2 * h * np.array([4.0, 0.25]) / 2, rtol=1e-13, atol=1e-18)
    np.testing.assert_allclose(r["grad_log_std"], [0.64, 0.16], atol=1e-5)


def test_samples_identity_and_the_deterministic_mode():
    c = sr.head_case(65, 129, np.float64)
    E = sr.resample(c["log_std"], sr.SEED, 3, 65)["E"]
    r = sr.act(c["mean"], c["latent"], c["log_std"], E, clip=(-0.3, 0.3))
    for e in range(65):
        assert abs((r["raw"][e] - c["mean"][e]) - float(c["latent"][e] @ E[e])) <= 1e-15 * max(1.0, r["abs_noise"][e])
    assert np.array_equal(r["action"], np.clip(r["raw"], -0.3, 0.3)) and (np.abs(r["raw"]) > 0.3).any()
    det = sr.act(c["mean"], c["latent"], c["log_std"], deterministic=True)
    assert np.array_equal(det["raw"], c["mean"]) and np.array_equal(det["entropy"], r["entropy"])
    np.testing.assert_allclose(det["logp"], -np.log(np.sqrt(r["V"])) - sr.HALF_LOG_2PI, rtol=1e-15)
    # the distribution's variance is what the samples have: over many matrices raw - mean has variance V - epsilon
    draws = np.stack([c["latent"][:4] @ sr.resample(c["log_std"], 9, k, 4)["E"].T for k in range(400)])
    got = np.array([draws[:, e, e].var() for e in range(4)])
    np.testing.assert_allclose(got, r["V"][:4] - sr.EPS, rtol=0.25)


def test_the_rng_keys_are_distinct_and_do_not_depend_on_the_shard():
    for L in (1, 2, 65, 1024):
        k = sr.keys(70, L)
        assert len(np.unique(k)) == k.size and int(k[69, L - 1]) == 69 * 1024 + L - 1
    assert len(np.unique(sr.keys(3, 1024))) == 3 * 1024 and int(sr.keys(2, 1024)[1, 0]) == int(sr.keys(1, 1024)[0, 1023]) + 1
    ls = sr.head_case(8, 233, np.float32)["log_std"]
    whole = sr.resample(ls, sr.SEED, 5, 70)["E"]
    assert np.array_equal(sr.resample(ls, sr.SEED, 5, 30, offset=40)["E"], whole[40:])
    assert np.array_equal(sr.resample(ls[:100], sr.SEED, 5, 70)["E"], whole[:, :100])          # nor on L
    other = sr.resample(ls, sr.SEED, 6, 70)["E"]
    assert not np.array_equal(other, whole) and abs(np.corrcoef(other.ravel(), whole.ravel())[0, 1]) < 0.02
    z = sr.resample(ls, sr.SEED, 5, 70)["z"]
    assert abs(z.mean()) < 0.03 and abs(z.std() - 1.0) < 0.03
    # the words are act_restatement's: element (e, k) draws what ptg_act's row (e * 1024 + k) would
    w0, w1 = ar.words(sr.SEED, 5, np.array([3 * 1024 + 7]))
    assert sr.resample(ls, sr.SEED, 5, 4)["z"][3, 7] == ar.normal(w0, w1)[0]
    bad = ls.copy(); bad[2] = np.nan; bad[5] = np.inf; bad[6] = -np.inf
    r = sr.resample(bad, 1, 0, 3)
    assert np.isnan(r["E"][:, [2, 5]]).all() and (r["E"][:, 6] == 0).all() and np.isfinite(np.delete(r["E"], [2, 5], axis=1)).all()


# ------------------------------------------------------------------------------------------------- the ABI, without a device
def test_the_library_exports_the_symbols_and_the_abi_stays_13():
    from rl_ptg_amd import _lib
    _lib.build()
    L = _lib.lib()
    names = ("ptg_sde_resample", "ptg_sde_act", "ptg_sde_policy_loss_workspace", "ptg_sde_policy_loss")
    assert all(hasattr(L, n) and n in _lib.EXPORTS for n in names)
    assert L.ptg_abi_version() == 13
    for d, f in ((_lib.PtgSdeNoise, L.ptg_sde_resample), (_lib.PtgSdeHead, L.ptg_sde_act), (_lib.PtgSdeLoss, L.ptg_sde_policy_loss)):
        assert f(None, C.byref(d()), None) == _lib.E_INVALID
    hdr = open(os.path.join(ROOT, "include", "ptg_env.h")).read()
    assert "Out of scope: the networks, gSDE" not in hdr and "caller reads stats[4]), gSDE" not in hdr


@pytest.mark.parametrize("name", ["ptg_sde_noise", "ptg_sde_head", "ptg_sde_loss"])
def test_the_struct_layouts_match_the_c_compiler(tmp_path, name):
    import subprocess
    from rl_ptg_amd import _lib
    S = {"ptg_sde_noise": _lib.PtgSdeNoise, "ptg_sde_head": _lib.PtgSdeHead, "ptg_sde_loss": _lib.PtgSdeLoss}[name]
    fs = [f for f, _ in S._fields_]
    body = 'printf("%%zu", sizeof(%s));\n' % name + "\n".join('printf(" %%zu", offsetof(%s, %s));' % (name, f) for f in fs)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){%s return 0;}\n' % (os.path.join(ROOT, "include", "ptg_env.h"), body))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in fs]
    assert C.sizeof(S) == {"ptg_sde_noise": 48, "ptg_sde_head": 120, "ptg_sde_loss": 224}[name]


def test_the_workspace_size_against_its_python_restatement():
    from rl_ptg_amd import _lib
    from rl_ptg_amd.train_ops import TrainOps
    W, P = _lib.lib().ptg_sde_policy_loss_workspace, TrainOps.sde_policy_loss_workspace_bytes
    assert W(1, 1) == 8 * (4 + 3 + 1 + 9) and W(203, 358) == 8 * (4 + 3 + 358 + 51 * 366)
    assert W(4096, 2) == 8 * (4 + 48 + 2 + 1024 * 10) and W(4097, 2) == 8 * (4 + 51 + 2 + 513 * 10)      # two rows a wave from there
    assert W(2 ** 31, 1024) == 8 * (4 + 3 * 2 ** 23 + 1024 + 1024 * 1032)
    rng = np.random.default_rng(5)
    for _ in range(300):
        B, L = int(rng.integers(1, 200000)), int(rng.integers(1, 1025))
        assert W(B, L) == P(B, L) > 0
    for bad in ((0, 5), (2 ** 31 + 1, 5), (4, 0), (4, 1025), (-3, 5)):
        assert W(*bad) < 0 and P(*bad) < 0


# ------------------------------------------------------------------------------------------------- the Python argument checks
def _loss_args(B=6, L=5, dt=None):
    import torch
    dt = torch.float32 if dt is None else dt
    z = lambda *s: torch.zeros(*s, dtype=dt)
    return dict(kind="ppo", mean=z(B), values=z(B), latent=z(B, L), log_std=z(L), actions=z(B), old_log_prob=z(B), advantages=z(B), returns=z(B), clip_range=0.2)


def test_python_argument_checks_need_no_device():
    import torch
    from helpers import host_engine
    from rl_ptg_amd.train_ops import SdeAct, SdePolicyLoss
    N, L, B = 4, 5, 6
    eng = host_engine(N)
    other = torch.device("meta")
    t, v = TypeError, ValueError
    z = torch.zeros
    cnt = z(1, dtype=torch.int64)
    res = lambda **kw: eng.sde_resample(**{**dict(log_std=z(L), counter=cnt, noise=z(N, L)), **kw})
    act = lambda **kw: eng.sde_act(**{**dict(mean=z(N), latent=z(N, L), log_std=z(L), noise=z(N, L)), **kw})
    loss = lambda **kw: eng.sde_policy_loss(**{**_loss_args(B, L), **kw})
    out_a = lambda **kw: SdeAct(**{**dict(actions=z(N), raw=z(N), log_prob=z(N), entropy=z(N)), **kw})
    out_l = lambda **kw: SdePolicyLoss(**{**dict(stats=z(8).double(), grad_input=z(B), grad_values=z(B), grad_log_std=z(L), grad_latent=None), **kw})
    need = eng.sde_policy_loss_workspace_bytes(B, L)
    refused = [
        # sde_resample
        (t, lambda: res(log_std=None)), (t, lambda: res(log_std=z(L).half())), (t, lambda: res(log_std=z(L).numpy())), (v, lambda: res(log_std=z(L, 2))),
        (v, lambda: res(log_std=z(2 * L)[::2])), (v, lambda: res(log_std=z(0))), (v, lambda: res(log_std=z(1025), noise=z(N, 1025))),
        (v, lambda: res(log_std=z(L, device=other))), (t, lambda: res(counter=None)), (t, lambda: res(counter=z(1))), (t, lambda: res(counter=z(2, dtype=torch.int64))),
        (v, lambda: res(noise=z(N, L).double())), (v, lambda: res(noise=z(N + 1, L))), (v, lambda: res(noise=z(N, L + 1))), (v, lambda: res(noise=z(L, N).t())),
        (v, lambda: res(noise=z(N, L, device=other))), (v, lambda: res(noise=None)),
        (t, lambda: res(log_std=z(L).half(), noise=z(N + 1, L))),                         # TypeError before the ValueError of another argument
        # sde_act
        (t, lambda: act(mean=None)), (t, lambda: act(mean=z(N).half())), (v, lambda: act(mean=z(N + 1))), (v, lambda: act(mean=z(N, 2))),
        (t, lambda: act(log_std=z(L).double())), (v, lambda: act(log_std=z(L + 1))), (t, lambda: act(latent=z(N, L).double())), (t, lambda: act(latent=None)),
        (v, lambda: act(latent=z(N, L + 1))), (v, lambda: act(latent=z(L, N).t())), (v, lambda: act(latent=z(N, L, device=other))),
        (v, lambda: act(noise=None)), (t, lambda: act(noise=z(N, L).double())), (v, lambda: act(noise=z(N - 1, L))), (v, lambda: act(clip=(1.0, -1.0))),
        (v, lambda: act(clip=(float("nan"), 1.0))), (v, lambda: act(out=out_a(actions=z(N).double()))), (v, lambda: act(out=out_a(raw=z(N + 1)))),
        (v, lambda: act(out=out_a(actions=None))), (v, lambda: act(out=out_a(), want_entropy=False)), (v, lambda: act(out=(z(N),))),
        (v, lambda: act(out=out_a(log_prob=z(2 * N)[::2]))),
        # sde_policy_loss
        (v, lambda: loss(kind="dqn")), (t, lambda: loss(mean=None)), (t, lambda: loss(mean=z(B).half())), (v, lambda: loss(mean=z(B, 2))), (v, lambda: loss(mean=z(0))),
        (t, lambda: loss(log_std=z(L).double())), (v, lambda: loss(log_std=z(L, 3))), (t, lambda: loss(latent=z(B, L).double())), (v, lambda: loss(latent=z(B + 1, L))),
        (v, lambda: loss(latent=z(B, L - 1))), (v, lambda: loss(latent=z(L, B).t())), (t, lambda: loss(values=z(B).double())), (v, lambda: loss(values=z(B + 1))),
        (v, lambda: loss(old_log_prob=None)), (v, lambda: loss(clip_range_vf=0.3)), (t, lambda: loss(actions=z(B).long())), (v, lambda: loss(actions=z(2 * B)[::2])),
        (t, lambda: loss(advantages=z(B).double())), (v, lambda: loss(returns=z(B - 1))), (v, lambda: loss(old_log_prob=z(B, device=other))),
        (t, lambda: loss(clip_range_vf=0.3, old_values=z(B).double())), (v, lambda: loss(clip_range=None)), (v, lambda: loss(clip_range=-0.1)),
        (v, lambda: loss(clip_range=float("nan"))), (v, lambda: loss(clip_range_vf=-1.0, old_values=z(B))),
        (v, lambda: loss(out=out_l(stats=z(8)))), (v, lambda: loss(out=out_l(stats=z(7).double()))), (v, lambda: loss(out=out_l(grad_input=z(B).double()))),
        (v, lambda: loss(out=out_l(grad_values=z(B + 1)))), (v, lambda: loss(out=out_l(grad_log_std=z(1)))), (v, lambda: loss(out=out_l(grad_log_std=None))),
        (v, lambda: loss(out=out_l(grad_latent=z(B, L + 1)))), (v, lambda: loss(out=out_l(grad_latent=z(L, B).t()))), (v, lambda: loss(out=(z(8).double(),))),
        (v, lambda: loss(workspace=z(need))), (v, lambda: loss(workspace=z(need - 1, dtype=torch.uint8))), (v, lambda: loss(workspace=z(2 * need, dtype=torch.uint8)[::2])),
        (t, lambda: loss(mean=z(B).half(), latent=z(B + 1, L))),
    ]
    assert len(refused) == 78
    for k, (exc, fn) in enumerate(refused):
        with pytest.raises(exc, match="sde_resample|sde_act|sde_policy_loss"):
            fn()
        assert eng._L is None, k
    with pytest.raises(ValueError, match="sde_policy_loss_workspace"):
        host_engine(N, _L=type("L", (), {"ptg_sde_policy_loss_workspace": staticmethod(lambda b, l: -1)})()).sde_policy_loss_workspace(0, 5)


def test_a_good_call_reaches_the_library_once_with_the_strides_it_was_given():
    import torch
    from helpers import recording_engine
    from rl_ptg_amd import _lib
    N, L, B = 4, 5, 6
    eng = recording_engine(N)
    z = torch.zeros
    ws = z(N, 16)                                             # a kept hidden layer: rows padded to 16 bytes and more
    lat, noise, out2 = ws[:, :L], z(N, 8)[:, :L], z(N, 2)
    cnt = z(1, dtype=torch.int64)
    eng.sde_resample(z(L, 1), cnt, noise, seed=-1)
    res = eng.sde_act(out2[:, 0], lat, z(L), noise, clip=(-0.5, 0.25))
    det = eng.sde_act(out2[:, :1], lat, z(L), None, deterministic=True, want_entropy=False)
    assert [c[0] for c in eng._L.calls] == ["ptg_sde_resample", "ptg_sde_act", "ptg_sde_act"]
    d = eng._L.calls[0][1][1]._obj
    assert (d.in_dtype, d.latent_dim, d.seed, d.counter_dev, d.e_dev, d.e_s_n) == (_lib.OUT_F32, L, 2 ** 64 - 1, cnt.data_ptr(), noise.data_ptr(), 8)
    d = eng._L.calls[1][1][1]._obj
    assert (d.flags, d.in_dtype, d.latent_dim, d.act_kind, d.mean_dev, d.mean_s_n) == (0, _lib.OUT_F32, L, _lib.ACT_F32, out2.data_ptr(), 2)
    assert (d.latent_dev, d.latent_s_n, d.e_dev, d.e_s_n, d.clip_lo, d.clip_hi) == (lat.data_ptr(), 16, noise.data_ptr(), 8, -0.5, 0.25)
    assert (d.act_dev, d.raw_dev, d.logp_dev, d.ent_dev) == tuple(t.data_ptr() for t in res) and res.actions.dtype == torch.float32
    d = eng._L.calls[2][1][1]._obj
    assert (d.flags, d.e_dev, d.e_s_n, d.ent_dev, d.mean_s_n) == (_lib.HEAD_DETERMINISTIC, None, 0, None, 2) and det.entropy is None
    eng._L.calls.clear()
    a = _loss_args(B, L, torch.float64)
    a.update(kind="a2c", latent=z(B, 8).double()[:, :L], mean=z(B, 2).double()[:, 1], old_log_prob=None, clip_range=None)
    r = eng.sde_policy_loss(**a, want_grad_latent=True, workspace=z(eng.sde_policy_loss_workspace_bytes(B, L), dtype=torch.uint8))
    assert [c[0] for c in eng._L.calls] == ["ptg_sde_policy_loss"]
    d = eng._L.calls[0][1][1]._obj
    assert (d.kind, d.flags, d.in_dtype, d.latent_dim, d.batch, d.mean_s_n, d.val_s_n, d.latent_s_n, d.old_logp_dev) == (_lib.LOSS_A2C, 0, _lib.OUT_F64, L, B, 2, 1, 8, None)
    assert (d.grad_latent_dev, d.gl_s_n, d.grad_log_std_dev) == (r.grad_latent.data_ptr(), L, r.grad_log_std.data_ptr())
    assert r.grad_log_std.shape == (L,) and r.grad_latent.shape == (B, L) and r.stats.dtype == torch.float64
