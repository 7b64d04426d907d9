"""What gSDE's ops for SAC / TQC (ptg_sde_resample_rows, ptg_sde_rsample, ptg_sde_rsample_backward) rest on that needs no GPU:
tests/sde_squash_restatement.py against SB3's own expressions under torch float64 autograd -- the row drawn by Normal(0, std).rsample(),
F.hardtanh, mm / bmm, tanh, the atanh(clamp(.)) round trip, log(1 - tanh^2 + 1e-6) -- for the action, the log-prob and all three
gradients; the exclusive Hardtanh gradient; a 2-row case by hand; the two paths into log_std apart; the shared row against B copies;
the key layout of the training row; the descriptor as gcc sees it; the workspace size; every Python-level refusal.

The bound against torch, derived.  SB3 recovers g as g' = atanh(y), y = tanh(g) rounded.  d atanh / d y = 1 / (1 - y^2) = cosh(g)^2, so
a relative error u = 2^-53 in y moves g' by |y| * u * cosh(g)^2; log1p(y), log1p(-y), their difference and the halving add as much
again (1 - |y| carries the same relative error u / (1 - |y|) <= u * cosh(g)^2 * 2), and autograd's d g' / d g, the product
(1 / (1 - y^2)) * (1 - y^2) from differently rounded factors, is 1 within the same relative amount.  With every |g| <= G (asserted; the
cases are drawn so, the clamp at 1 - 2^-52 is then inactive by a wide margin: 1 - tanh(3.5) = 1.8e-3):
    eps_g = 8 * 2^-53 * cosh(G)^2                            (both the absolute error of g' and the relative error of d g' / d g)
g' enters log_prob as (g' - m)^2 / (2 V), whose derivative is noise / V per unit of g', and the gradients as gl * (g' - m) / V (the
mean and noise paths) and gl * (g' - m)^2 / (2 V^2) (the variance path, times 2 h s^2 <= 2 V / |h| ... bounded here by 2 / V_min per
unit).  So with amp = max_i (1 + |noise_i|) / V_i and vamp = max(1, 1 / V_min):
    se = L * 2^-53 * max(1, sum |term| of noise, of V)       (torch's mm / bmm add the L terms in another order than the lanes do)
    |act - ref| <= 4 * 2^-53 + se                            (tanh alone, no round trip; d a / d noise <= 1)
    |logp - ref| <= (eps_g + se) * amp * (1 + G)  + 1e-14 * max |ref|
    gradients: |x - ref| <= (eps_g + se) * amp * vamp * (1 + G) * scale + 1e-14 * max |ref|,   scale = max(|ga|, |gl|) * max(1, |E|, |h|),
    times B for grad_log_std, a sum of B such terms.
The bound is computed per case from the case's reference V and noise and printed beside the measured error; on the cases below it lies
between 1e-11 and 1e-9 of the incoming scale, which is this check's resolution -- the conditioning of atanh(tanh(g)), not the
restatement's."""
import ctypes as C
import os

import numpy as np
import pytest

import act_restatement as ar
import sde_restatement as sr
import sde_squash_restatement as sq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 3.5
U53 = 2.0 ** -53
EPS_G = 8 * U53 * np.cosh(G) ** 2


def host_case(B, L, seed=0):
    """float64; V of about 0.15 whatever L (log_std around log(0.6 / sqrt(L))), |latent| in [0.3, 1), means in [-2.4, 2.4] with the first
    six rows at clip_mean exactly, one spacing inside and one outside on either side: |g| stays below G"""
    rng = np.random.default_rng([B, L, 41, seed])
    ls = np.log(0.6 / np.sqrt(L)) + rng.uniform(-0.3, 0.3, L)
    h = rng.uniform(0.3, 1.0, (B, L)) * rng.choice([-1.0, 1.0], (B, L))
    mu = rng.uniform(-2.4, 2.4, B)
    edge = [2.0, -2.0, np.nextafter(2.0, 0.0), np.nextafter(2.0, 3.0), np.nextafter(-2.0, 0.0), np.nextafter(-2.0, -3.0)]
    mu[:min(B, 6)] = edge[:min(B, 6)]
    s = np.exp(ls)
    z = np.clip(rng.standard_normal(L), -2.0, 2.0)
    zm = np.clip(rng.standard_normal((B, L)), -2.0, 2.0)
    w = rng.standard_normal(B)
    return dict(mean=mu, latent=h, log_std=ls, row=s * z, matrix=s[None, :] * zm, w=w, grad_act=-w / B, grad_logp=np.full(B, sq.ENT_COEF / B))


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("B,L", [(1, 1), (2, 2), (6, 65), (203, 233), (290, 708), (257, 129)])
def test_the_restatement_against_sb3s_expressions_under_autograd(B, L, shared):
    c = host_case(B, L)
    E = c["row"] if shared else c["matrix"]
    f = sq.forward(c["mean"], c["latent"], c["log_std"], E)
    b = sq.backward(c["mean"], c["latent"], c["log_std"], E, f["saved"], c["grad_act"], c["grad_logp"])
    t = sq.torch_reference(c, E, shared=shared)
    assert not f["bad"].any() and not b["bad"].any() and np.abs(f["g"]).max() <= G, np.abs(f["g"]).max()
    amp = float(((1.0 + np.abs(f["noise"])) / f["V"]).max())
    vamp = max(1.0, 1.0 / float(f["V"].min()))
    scale = max(np.abs(c["grad_act"]).max(), np.abs(c["grad_logp"]).max()) * max(1.0, np.abs(E).max(), np.abs(c["latent"]).max())
    r14 = lambda k: 1e-14 * float(np.abs(t[k]).max())
    se = L * U53 * max(1.0, float(f["abs_noise"].max()), float(f["abs_V"].max()))       # mm / bmm add the L terms in another order
    eg = EPS_G + se
    bounds = dict(act=4 * U53 + se, logp=eg * amp * (1 + G) + r14("logp"), grad_mean=eg * amp * vamp * (1 + G) * scale + r14("grad_mean"),
                  grad_latent=eg * amp * vamp * (1 + G) * scale + r14("grad_latent"))
    got = dict(act=f["act"], logp=f["logp"], grad_mean=b["grad_mean"], grad_latent=b["grad_latent"])
    if shared:
        bounds["grad_log_std"] = B * eg * amp * vamp * (1 + G) * scale + r14("grad_log_std")
        got["grad_log_std"] = b["grad_log_std"]
    worst = {k: float(np.abs(got[k] - t[k]).max()) / bounds[k] for k in bounds}
    print(f"B={B} L={L} shared={shared}: bounds", {k: f"{v:.2e}" for k, v in bounds.items()}, "error / bound", {k: round(v, 4) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst


def test_hardtanhs_gradient_is_exclusive_at_both_ends():
    """torch's F.hardtanh passes the gradient where -c < mu < c and nowhere else; the restatement's line says the same"""
    import torch
    import torch.nn.functional as F
    c = host_case(6, 5)
    mu = torch.from_numpy(c["mean"]).requires_grad_(True)
    F.hardtanh(mu, -2.0, 2.0).sum().backward()
    assert mu.grad.tolist() == [0.0, 0.0, 1.0, 0.0, 1.0, 0.0]
    f = sq.forward(c["mean"], c["latent"], c["log_std"], c["row"])
    b = sq.backward(c["mean"], c["latent"], c["log_std"], c["row"], f["saved"], c["grad_act"], c["grad_logp"])
    assert ((b["grad_mean"] != 0) == (mu.grad.numpy() != 0)).all() and np.array_equal(b["grad_mean"][[2, 4]], b["t"][[2, 4]])
    assert np.array_equal(f["m"], [2.0, -2.0, c["mean"][2], 2.0, c["mean"][4], -2.0])
    free = sq.backward(c["mean"], c["latent"], c["log_std"], c["row"], sq.forward(c["mean"], c["latent"], c["log_std"], c["row"], clip_mean=np.inf)["saved"],
                       c["grad_act"], c["grad_logp"], clip_mean=np.inf)
    assert (free["grad_mean"] != 0).all()


def test_two_rows_by_hand():
    """L = 2, log_std = log([2, 1/2]) so s^2 = [4, 1/4]; rows h = [1, 2] and [0, 4]; E = [0.5, -0.25]; mu = [0.25, 3] (the second clipped to 2)"""
    ls = np.log(np.array([2.0, 0.5]))
    h = np.array([[1.0, 2.0], [0.0, 4.0]])
    E = np.array([0.5, -0.25])
    mu = np.array([0.25, 3.0])
    ga, gl = np.array([1.0, -2.0]), np.array([0.5, 0.25])
    f = sq.forward(mu, h, ls, E)
    V = np.array([5.0 + 1e-6, 4.0 + 1e-6])                   # 1 * 4 + 4 / 4 and 16 / 4, plus epsilon
    noise = np.array([0.0, -1.0])                            # 0.5 - 0.5 and -0.25 * 4
    np.testing.assert_allclose(f["V"], V, rtol=1e-15)
    assert np.array_equal(f["noise"], noise) and np.array_equal(f["g"], [0.25, 1.0])
    a = np.tanh([0.25, 1.0])
    np.testing.assert_allclose(f["act"], a, rtol=1e-15)
    np.testing.assert_allclose(f["logp"], -noise ** 2 / (2 * V) - 0.5 * np.log(V) - 0.5 * np.log(2 * np.pi) - np.log(1 - a ** 2 + 1e-6), rtol=1e-14)
    b = sq.backward(mu, h, ls, E, f["saved"], ga, gl)
    d = 1 - a ** 2
    q = 2 * a * d / (d + 1e-6)
    t = ga * d + gl * q
    np.testing.assert_allclose(b["grad_mean"], [t[0], 0.0], rtol=1e-14)
    n = t - gl * noise / V                                   # row 0: t; row 1: t + 0.25 / 4
    cV = gl * (noise ** 2 / V - 1) / (2 * V)                 # row 0: -0.05; row 1: 0.25 * (1 / 4 - 1) / 8 = -0.0234375, up to epsilon
    np.testing.assert_allclose(cV, [-0.05, -0.0234375], atol=1e-7)
    g_lat = n[:, None] * E[None, :] + cV[:, None] * 2 * h * np.array([4.0, 0.25])
    np.testing.assert_allclose(b["grad_latent"], g_lat, rtol=1e-13)
    np.testing.assert_allclose(b["grad_log_std"], (h * g_lat).sum(axis=0), rtol=1e-13)
    np.testing.assert_allclose(b["grad_log_std"][0], 1.0 * (t[0] * 0.5 - 0.05 * 2 * 4), rtol=1e-6)      # only row 0 has h_0 != 0


@pytest.mark.parametrize("B,L", [(5, 65), (203, 233), (4100, 3)])
def test_the_log_std_gradient_is_the_variance_path_plus_the_matrix_path(B, L):
    c = host_case(B, L)
    f = sq.forward(c["mean"], c["latent"], c["log_std"], c["row"])
    b = sq.backward(c["mean"], c["latent"], c["log_std"], c["row"], f["saved"], c["grad_act"], c["grad_logp"])
    both = b["variance_path"] + b["matrix_path"]
    assert np.abs(both - b["grad_log_std"]).max() <= (B * U53 + 1e-14) * np.maximum(1.0, b["abs_gls"]).max()
    assert np.abs(b["variance_path"]).max() > 0 and np.abs(b["matrix_path"]).max() > 0
    # the matrix path alone is what autograd sends through Normal(0, std).rsample(): E_k * d loss / d E_k
    np.testing.assert_allclose(b["matrix_path"], c["row"] * (b["n"][:, None] * c["latent"]).sum(axis=0), rtol=1e-13)
    # the sums' orders: batch_sum and wave_sum against NumPy's
    assert np.abs(sq.batch_sum(c["latent"]) - c["latent"].sum(axis=0)).max() <= B * U53 * np.abs(c["latent"]).sum(axis=0).max()
    assert np.abs(sq.wave_sum(c["latent"]) - c["latent"].sum(axis=1)).max() <= L * U53 * np.abs(c["latent"]).sum(axis=1).max()


def test_the_shared_row_equals_the_per_row_call_on_copies_bit_for_bit():
    for B, L in ((1, 1), (7, 65), (257, 233)):
        c = sq.case(B, L, np.float64)
        one = sq.forward(c["mean"], c["latent"], c["log_std"], c["row"])
        many = sq.forward(c["mean"], c["latent"], c["log_std"], np.tile(c["row"], (B, 1)))
        for k in ("act", "logp", "saved"):
            assert np.array_equal(one[k].view(np.int64), many[k].view(np.int64)), k
        det = sq.forward(c["mean"], c["latent"], c["log_std"], deterministic=True)
        assert np.array_equal(det["act"], np.tanh(sq.hardtanh(c["mean"].astype(np.float64), 2.0))) and np.array_equal(det["V"], one["V"])


def test_the_training_rows_keys_have_no_env_offset_and_their_own_stream():
    from rl_ptg_amd import sde
    assert sde.TRAIN_SEED_XOR == sq.TRAIN_SEED_XOR == 0x9E3779B97F4A7C15
    ls = sr.head_case(8, 233, np.float32)["log_std"]
    rows = sq.resample_rows(ls, sr.SEED, 5, 7)
    assert np.array_equal(rows["E"], sr.resample(ls, sr.SEED, 5, 7, offset=0)["E"])         # the collecting keys at offset 0 ...
    assert not np.array_equal(rows["E"], sr.resample(ls, sr.SEED, 5, 7, offset=4000)["E"])  # ... and never a shard's
    w0, w1 = ar.words(sr.SEED, 5, np.array([3 * 1024 + 7]))
    assert rows["z"][3, 7] == ar.normal(w0, w1)[0]
    # SquashedSdeNoise: at equal seed and equal counter values the training row is no row of the collecting matrix
    train = sq.resample_rows(ls, sr.SEED ^ sq.TRAIN_SEED_XOR, 0, 1)["E"][0]
    collect = sr.resample(ls, sr.SEED, 0, 64)["E"]
    assert not (collect == train[None, :]).all(axis=1).any() and abs(np.corrcoef(collect[0], train)[0, 1]) < 0.2
    assert (sr.SEED ^ sq.TRAIN_SEED_XOR) != sr.SEED and 0 <= (sr.SEED ^ sq.TRAIN_SEED_XOR) < 2 ** 64


# ------------------------------------------------------------------------------------------------- the ABI, without a device
def test_the_library_exports_the_symbols_and_the_abi_stays_13():
    from rl_ptg_amd import _lib
    _lib.build()
    L = _lib.lib()
    names = ("ptg_sde_resample_rows", "ptg_sde_rsample", "ptg_sde_rsample_backward", "ptg_sde_rsample_backward_workspace")
    assert all(hasattr(L, n) and n in _lib.EXPORTS for n in names)
    assert L.ptg_abi_version() == 13
    assert L.ptg_sde_resample_rows(None, C.byref(_lib.PtgSdeNoise()), 1, None) == _lib.E_INVALID
    for f in (L.ptg_sde_rsample, L.ptg_sde_rsample_backward):
        assert f(None, C.byref(_lib.PtgSdeRs()), None) == _lib.E_INVALID
    hdr = open(os.path.join(ROOT, "include", "ptg_env.h")).read()
    assert "Out of scope: SAC / TQC with gSDE" not in hdr
    assert (_lib.SDE_RS_DETERMINISTIC, _lib.SDE_RS_SHARED_E) == (1, 2) and "PTG_SDE_RS_DETERMINISTIC = 1, PTG_SDE_RS_SHARED_E = 2" in hdr


def test_the_struct_layout_matches_the_c_compiler(tmp_path):
    import subprocess
    from rl_ptg_amd import _lib
    S, name = _lib.PtgSdeRs, "ptg_sde_rs"
    fs = [f for f, _ in S._fields_]
    body = 'printf("%%zu", sizeof(%s));\n' % name + "\n".join('printf(" %%zu", offsetof(%s, %s));' % (name, f) for f in fs)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){%s return 0;}\n' % (os.path.join(ROOT, "include", "ptg_env.h"), body))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in fs]
    assert C.sizeof(S) == 184


def test_the_workspace_size_against_its_python_restatement():
    from rl_ptg_amd import _lib
    from rl_ptg_amd.train_ops import TrainOps
    W, P = _lib.lib().ptg_sde_rsample_backward_workspace, TrainOps.sde_rsample_backward_workspace_bytes
    assert W(1, 1) == 8 * 2 and W(203, 358) == 8 * 358 * 52 and W(470, 233) == 8 * 233 * 119
    assert W(4096, 2) == 8 * 2 * 1025 and W(4097, 2) == 8 * 2 * 514                      # two rows a wave from there
    assert W(2 ** 31, 1024) == 8 * 1024 * 1025
    rng = np.random.default_rng(5)
    for _ in range(300):
        B, L = int(rng.integers(1, 200000)), int(rng.integers(1, 1025))
        assert W(B, L) == P(B, L) > 0
    for bad in ((0, 5), (2 ** 31 + 1, 5), (4, 0), (4, 1025), (-3, 5)):
        assert W(*bad) < 0 and P(*bad) < 0


# ------------------------------------------------------------------------------------------------- the Python argument checks
def test_python_argument_checks_need_no_device():
    import torch
    from helpers import host_engine
    from rl_ptg_amd.train_ops import SdeRSample, SdeRSampleGrad
    N, L, B = 4, 5, 6
    eng = host_engine(N)
    other = torch.device("meta")
    t, v = TypeError, ValueError
    z = torch.zeros
    cnt = z(1, dtype=torch.int64)
    inf, nan = float("inf"), float("nan")
    res = lambda **kw: eng.sde_resample_rows(**{**dict(log_std=z(L), counter=cnt, noise=z(L)), **kw})
    fwd = lambda **kw: eng.sde_rsample(**{**dict(mean=z(B), latent=z(B, L), log_std=z(L), noise=z(L)), **kw})
    bwd = lambda **kw: eng.sde_rsample_backward(**{**dict(mean=z(B), latent=z(B, L), log_std=z(L), noise=z(L), saved=z(B, 2).double(), grad_actions=z(B),
                                                          grad_log_prob=z(B)), **kw})
    out_f = lambda **kw: SdeRSample(**{**dict(actions=z(B), step_actions=z(B), log_prob=z(B), saved=z(B, 2).double()), **kw})
    out_b = lambda **kw: SdeRSampleGrad(**{**dict(grad_mean=z(B), grad_latent=z(B, L), grad_log_std=z(L)), **kw})
    need = eng.sde_rsample_backward_workspace_bytes(B, L)
    refused = [
        # sde_resample_rows
        (t, lambda: res(log_std=None)), (t, lambda: res(log_std=z(L).half())), (v, lambda: res(log_std=z(L, 2))), (v, lambda: res(log_std=z(0), noise=z(0))),
        (v, lambda: res(log_std=z(1025), noise=z(1025))), (t, lambda: res(counter=None)), (t, lambda: res(counter=z(1))), (v, lambda: res(noise=z(L).double())),
        (v, lambda: res(noise=z(L + 1))), (v, lambda: res(noise=z(3, L + 1))), (v, lambda: res(noise=z(0, L))), (v, lambda: res(noise=z(L, 3).t())),
        (v, lambda: res(noise=None)), (v, lambda: res(noise=z(L, device=other))),
        # sde_rsample
        (t, lambda: fwd(mean=None)), (t, lambda: fwd(mean=z(B).half())), (v, lambda: fwd(mean=z(B, 2))), (v, lambda: fwd(mean=z(0), latent=z(0, L))),
        (t, lambda: fwd(log_std=z(L).double())), (v, lambda: fwd(log_std=z(L + 1))), (t, lambda: fwd(latent=z(B, L).double())), (t, lambda: fwd(latent=None)),
        (v, lambda: fwd(latent=z(B + 1, L))), (v, lambda: fwd(latent=z(L, B).t())), (v, lambda: fwd(latent=z(B, L, device=other))), (v, lambda: fwd(noise=None)),
        (t, lambda: fwd(noise=z(L).double())), (v, lambda: fwd(noise=z(L + 1))), (v, lambda: fwd(noise=z(2 * L)[::2])), (v, lambda: fwd(noise=z(B - 1, L))),
        (v, lambda: fwd(noise=z(L, B).t())), (v, lambda: fwd(clip_mean=0.0)), (v, lambda: fwd(clip_mean=-2.0)), (v, lambda: fwd(clip_mean=nan)),
        (v, lambda: fwd(out=out_f(actions=None))), (v, lambda: fwd(out=out_f(actions=z(B).double()))), (v, lambda: fwd(out=out_f(step_actions=z(B).double()))),
        (v, lambda: fwd(out=out_f(log_prob=z(B + 1)))), (v, lambda: fwd(out=out_f(saved=z(B, 2)))), (v, lambda: fwd(out=out_f(saved=z(B, 3).double()))),
        (v, lambda: fwd(out=(z(B),))),
        # sde_rsample_backward
        (t, lambda: bwd(mean=z(B).half())), (t, lambda: bwd(latent=z(B, L).double())), (v, lambda: bwd(noise=None)), (t, lambda: bwd(saved=z(B, 2))),
        (t, lambda: bwd(saved=None)), (v, lambda: bwd(saved=z(B + 1, 2).double())), (v, lambda: bwd(saved=z(B, 4).double()[:, ::2])),
        (v, lambda: bwd(grad_actions=None, grad_log_prob=None)), (t, lambda: bwd(grad_actions=z(B).double())), (v, lambda: bwd(grad_log_prob=z(B + 1))),
        (v, lambda: bwd(grad_actions=z(2 * B)[::2])), (v, lambda: bwd(noise=z(B, L))),          # a matrix has no log_std gradient
        (v, lambda: bwd(noise=None, deterministic=True)),                                        # nor has no noise at all
        (v, lambda: bwd(clip_mean=0.0)), (v, lambda: bwd(out=out_b(grad_mean=z(B).double()))), (v, lambda: bwd(out=out_b(grad_latent=z(B, L + 1)))),
        (v, lambda: bwd(out=out_b(grad_latent=z(L, B).t()))), (v, lambda: bwd(out=out_b(grad_log_std=z(L + 1)))), (v, lambda: bwd(out=(z(B),))),
        (v, lambda: bwd(noise=z(B, L), out=out_b())), (v, lambda: bwd(workspace=z(need))), (v, lambda: bwd(workspace=z(need - 1, dtype=torch.uint8))),
        (v, lambda: bwd(workspace=z(2 * need, dtype=torch.uint8)[::2])), (t, lambda: bwd(mean=z(B).half(), latent=z(B + 1, L))),
    ]
    assert len(refused) == 65
    for k, (exc, fn) in enumerate(refused):
        with pytest.raises(exc, match="sde_resample_rows|sde_rsample|sde_rsample_backward"):
            fn()
        assert eng._L is None, k
    assert cnt.item() == 0
    with pytest.raises(ValueError, match="sde_rsample_backward_workspace"):
        host_engine(N, _L=type("L", (), {"ptg_sde_rsample_backward_workspace": staticmethod(lambda b, l: -1)})()).sde_rsample_backward_workspace(0, 5)


def test_a_good_call_reaches_the_library_once_with_the_strides_it_was_given():
    import torch
    from helpers import recording_engine
    from rl_ptg_amd import _lib
    N, L, B = 4, 5, 6
    eng = recording_engine(N)
    z = torch.zeros
    lat, out2, row, mat = z(B, 16)[:, :L], z(B, 2), z(L), z(B, 8)[:, :L]
    cnt = z(1, dtype=torch.int64)
    eng.sde_resample_rows(z(L, 1), cnt, row, seed=-1)
    eng.sde_resample_rows(z(L), cnt, mat)
    f = eng.sde_rsample(out2[:, 0], lat, z(L), row, want_step_actions=True)
    g = eng.sde_rsample(out2[:, :1], lat, z(L), mat, clip_mean=float("inf"), want_logp=False, want_saved=False)
    det = eng.sde_rsample(out2[:, 0], lat, z(L), None, deterministic=True)
    ws = z(eng.sde_rsample_backward_workspace_bytes(B, L), dtype=torch.uint8)
    b = eng.sde_rsample_backward(out2[:, 0], lat, z(L), row, f.saved, None, z(B), workspace=ws)
    m = eng.sde_rsample_backward(out2[:, 0], lat, z(L), mat, f.saved, z(B), None, want_grad_log_std=False, want_grad_latent=False, workspace=ws)
    assert [c[0] for c in eng._L.calls] == ["ptg_sde_resample_rows"] * 2 + ["ptg_sde_rsample"] * 3 + ["ptg_sde_rsample_backward"] * 2
    d, rows = eng._L.calls[0][1][1]._obj, eng._L.calls[0][1][2]
    assert (d.in_dtype, d.latent_dim, d.seed, d.counter_dev, d.e_dev, d.e_s_n, rows) == (_lib.OUT_F32, L, 2 ** 64 - 1, cnt.data_ptr(), row.data_ptr(), L, 1)
    d, rows = eng._L.calls[1][1][1]._obj, eng._L.calls[1][1][2]
    assert (d.e_dev, d.e_s_n, rows) == (mat.data_ptr(), 8, B)
    d = eng._L.calls[2][1][1]._obj
    assert (d.flags, d.in_dtype, d.latent_dim, d.batch, d.mean_dev, d.mean_s_n, d.latent_s_n, d.e_dev, d.e_s_n, d.clip_mean) == \
        (_lib.SDE_RS_SHARED_E, _lib.OUT_F32, L, B, out2.data_ptr(), 2, 16, row.data_ptr(), 0, 2.0)
    assert (d.act_dev, d.step_act_dev, d.logp_dev, d.saved_dev) == tuple(x.data_ptr() for x in f) and f.step_actions.dtype == torch.float32 and f.saved.shape == (B, 2)
    d = eng._L.calls[3][1][1]._obj
    assert (d.flags, d.e_dev, d.e_s_n, d.clip_mean, d.logp_dev, d.saved_dev, d.step_act_dev) == (0, mat.data_ptr(), 8, float("inf"), None, None, None) and g.log_prob is None
    d = eng._L.calls[4][1][1]._obj
    assert (d.flags, d.e_dev, d.e_s_n) == (_lib.SDE_RS_DETERMINISTIC, None, 0) and det.saved is not None
    d = eng._L.calls[5][1][1]._obj
    assert (d.flags, d.saved_dev, d.grad_act_dev, d.grad_logp_dev is not None, d.grad_mean_dev, d.gm_s_n) == (_lib.SDE_RS_SHARED_E, f.saved.data_ptr(), None, True, b.grad_mean.data_ptr(), 1)
    assert (d.grad_latent_dev, d.gl_s_n, d.grad_log_std_dev, d.ws_dev) == (b.grad_latent.data_ptr(), L, b.grad_log_std.data_ptr(), ws.data_ptr())
    d = eng._L.calls[6][1][1]._obj
    assert (d.flags, d.e_s_n, d.grad_latent_dev, d.gl_s_n, d.grad_log_std_dev) == (0, 8, None, 0, None) and m.grad_latent is None and m.grad_log_std is None
