"""The NumPy restatement of the action heads (tests/act_restatement.py) pinned by hand, its draw tested as a distribution, every input
of the GPU tests vetted (no ambiguous row), and the parts of ptg_act that need no device: the struct's size, the null handle, the
Python argument checks.  The restatement's own pins need nothing of the library (they stand on tests/act_restatement.py alone); the
struct-size, null-handle, error-code and argument-check tests need ptg_act and the act_* methods."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import act_restatement as ar
import replay_restatement as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LN2 = math.log(2.0)


def _w(u_hi):
    """(w0, w1) whose 53-bit uniform is u_hi / 2^32"""
    return np.array([u_hi], np.uint64), np.array([0], np.uint64)


def test_two_equal_logits_by_hand():
    """logits (0, 0): e = (1, 1), s = 2, both log-probs -ln 2, entropy ln 2; u * 2 < 1 iff u < 1/2"""
    for u_hi, want in ((0, 0), (2 ** 31 - 1, 0), (2 ** 31, 1), (2 ** 32 - 1, 1)):
        r = ar.categorical(np.zeros((1, 2)), *_w(u_hi))
        assert r["action"][0] == want and r["logp"][0] == -LN2 and r["entropy"][0] == LN2 and not r["bad"][0]
    assert ar.categorical(np.zeros((1, 2)), *_w(2 ** 31))["ambiguous"][0]            # u * s sits on the partial sum 1
    assert not ar.categorical(np.zeros((1, 2)), *_w(2 ** 30))["ambiguous"][0]
    d = ar.categorical(np.zeros((1, 2)), deterministic=True)
    assert d["action"][0] == 0 and d["logp"][0] == -LN2                              # the first maximal logit


def test_a_minus_inf_logit_is_probability_zero():
    """logits (0, -Inf): always action 0, log-prob 0, entropy 0 (the e_j == 0 term is left out, not 0 * -Inf)"""
    x = np.array([[0.0, -np.inf]])
    for u_hi in (0, 2 ** 31, 2 ** 32 - 1):
        r = ar.categorical(x, *_w(u_hi))
        assert r["action"][0] == 0 and r["logp"][0] == 0.0 and r["entropy"][0] == 0.0 and not r["bad"][0]
    r = ar.categorical(np.array([[-np.inf, -2.0, -np.inf]]), *_w(5))
    assert r["action"][0] == 1 and r["logp"][0] == 0.0


def test_three_logits_by_hand():
    """logits (ln 1, ln 2, ln 5) -> p = (1/8, 1/4, 5/8); the partial sums of e = (0.2, 0.4, 1) are 0.2, 0.6, 1.6"""
    x = np.log(np.array([[1.0, 2.0, 5.0]]))
    for u, want in ((0.1, 0), (0.13, 1), (0.37, 1), (0.38, 2), (0.99, 2)):
        r = ar.categorical(x, *_w(int(u * 2 ** 32)))
        assert r["action"][0] == want, u
        assert abs(r["logp"][0] - math.log([1 / 8, 1 / 4, 5 / 8][want])) < 1e-15
        assert abs(r["entropy"][0] - (math.log(8) / 8 + math.log(4) / 4 + 5 / 8 * math.log(8 / 5))) < 1e-15


def test_bad_rows():
    x = np.array([[0.0, 1.0], [np.nan, 0.0], [0.0, np.inf], [-np.inf, -np.inf], [0.0, -np.inf]])
    w0, w1 = ar.words(1, 0, np.arange(5))
    r = ar.categorical(x, w0, w1)
    assert r["bad"].tolist() == [False, True, True, True, False]
    assert (r["action"][1:4] == 0).all() and np.isnan(r["logp"][1:4]).all() and np.isnan(r["entropy"][1:4]).all()
    assert np.isfinite(r["logp"][[0, 4]]).all()
    q = ar.eps_greedy(x, 0.5, w0, w1)
    assert q["bad"].tolist() == [False, True, True, True, False]
    for eps in (float("nan"), -0.01, 1.0000001):
        assert ar.eps_greedy(x, eps, w0, w1)["bad"].all() and (ar.eps_greedy(x, eps, w0, w1)["action"] == 0).all()
    g = ar.gaussian(np.array([0.0, np.nan, np.inf, 0.0, 0.0, 0.0]), np.array([0.0, 0.0, 0.0, np.nan, np.inf, -np.inf]), *ar.words(1, 0, np.arange(6)))
    assert g["bad"].tolist() == [False, True, True, True, True, False]
    assert (g["action"][1:5] == 0).all() and np.isnan(g["raw"][1:5]).all() and np.isnan(g["logp"][1:5]).all() and np.isnan(g["entropy"][1:5]).all()


def test_one_typed_out_key_and_the_replay_chain():
    """(seed, c, e) = (0x0123456789ABCDEF, 3, 2^32 + 5): every 32-bit half of the key is used; the replay restatement's draw with
    total = 2^64 is the 64-bit word itself"""
    seed, c, e = 0x0123456789ABCDEF, 3, 0x100000005
    w0, w1 = ar.words(seed, c, [e])
    assert (int(w0[0]), int(w1[0])) == (0xF4AEAB5F, 0x3743CBE0)
    assert rr.draw_index(seed, c, e, 2 ** 64) == 0xF4AEAB5F3743CBE0
    g = np.array([0, 1, 63, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 7])
    w0, w1 = ar.words(7, 2 ** 33 + 1, g)
    assert [(int(a) << 32) | int(b) for a, b in zip(w0, w1)] == [rr.draw_index(7, 2 ** 33 + 1, int(b), 2 ** 64) for b in g]
    assert w0.max() < 2 ** 32 and w1.max() < 2 ** 32


def test_eps_greedy_by_hand():
    q = np.array([[1.0, 3.0, 3.0, -2.0]] * 6)
    w0 = np.array([0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 12345], np.uint64)
    w1 = np.array([0, 2 ** 30, 2 ** 31, 2 ** 32 - 1, 3 * 2 ** 30, 2 ** 30 - 1], np.uint64)
    assert ar.eps_threshold(0.5) == 2 ** 31 and ar.eps_threshold(0.0) == 0 and ar.eps_threshold(1.0) == 2 ** 32
    r = ar.eps_greedy(q, 0.0, w0, w1)
    assert not r["explore"].any() and (r["action"] == 1).all()                  # never explores; the tie goes to the first maximum
    r = ar.eps_greedy(q, 1.0, w0, w1)
    assert r["explore"].all() and r["action"].tolist() == [0, 1, 2, 3, 3, 0]     # always explores: (w1 * 4) >> 32
    r = ar.eps_greedy(q, 0.5, w0, w1)
    assert r["explore"].tolist() == [True, True, True, False, False, True]       # w0 < 2^31 exactly
    assert r["action"].tolist() == [0, 1, 2, 1, 1, 0]
    assert (ar.eps_greedy(q, deterministic=True)["action"] == 1).all()


def test_gaussian_by_hand():
    """w0 = 2^32 - 1 gives u1 = 1, z = 0: the sample is the mean; w1 = 0 gives cos 0 = 1, z = sqrt(-2 ln u1)"""
    top = np.array([2 ** 32 - 1], np.uint64)
    zero = np.array([0], np.uint64)
    assert ar.normal(top, zero)[0] == 0.0
    assert ar.normal(zero, zero)[0] == math.sqrt(64 * LN2) and ar.normal(zero, zero)[0] < 6.67          # the largest |z|
    w0 = np.array([int(math.exp(-0.5) * 2 ** 32) - 1], np.uint64)                                     # u1 = e^-1/2 -> z = 1 (to 2^-32)
    r = ar.gaussian(np.array([0.25]), np.array([math.log(0.5)]), w0, zero, clip=(-0.5, 0.5))
    assert abs(r["raw"][0] - 0.75) < 1e-9 and r["action"][0] == 0.5
    assert abs(r["logp"][0] - (-0.5 - math.log(0.5) - 0.5 * math.log(2 * math.pi))) < 1e-9
    assert r["entropy"][0] == 1.4189385332046727 + math.log(0.5) and abs(1.4189385332046727 - (0.5 + 0.5 * math.log(2 * math.pi))) < 1e-15
    s = ar.gaussian(np.array([0.25]), np.array([math.log(0.5)]), w0, zero, squash=True)
    a = math.tanh(r["raw"][0])
    assert abs(s["action"][0] - a) < 1e-15 and s["entropy"] is None and abs(s["logp"][0] - (r["logp"][0] - math.log(1 - a * a + 1e-6))) < 1e-14
    d = ar.gaussian(np.array([0.25]), np.array([0.0]), deterministic=True)
    assert d["raw"][0] == 0.25 and d["logp"][0] == -ar.HALF_LOG_2PI


N_DRAWS = 200000


@pytest.fixture(scope="module")
def many_words():
    return ar.words(2, 0, np.arange(N_DRAWS))                # seed 2: chosen here, on the CPU, among 0, 1, 2 (all three pass)


def test_categorical_draws_follow_the_distribution(many_words):
    """200 000 draws from one 5-way distribution: chi^2 over 4 degrees of freedom below 18.47, the 0.999 quantile"""
    row = np.array([0.3, -1.2, 2.0, 0.0, -0.5])
    r = ar.categorical(np.tile(row, (N_DRAWS, 1)), *many_words)
    p = np.exp(row - row.max()); p /= p.sum()
    counts = np.bincount(r["action"], minlength=5)
    chi2 = float(((counts - N_DRAWS * p) ** 2 / (N_DRAWS * p)).sum())
    assert counts.sum() == N_DRAWS and chi2 < 18.47, (counts, chi2)
    assert r["ambiguous"].sum() == 0


def test_normal_draws_have_mean_zero_and_variance_one(many_words):
    z = ar.normal(*many_words)
    assert abs(z.mean()) < 4 / math.sqrt(N_DRAWS) and abs(z.var() - 1) < 4 * math.sqrt(2 / N_DRAWS), (z.mean(), z.var())
    assert np.abs(z).max() <= 6.66


def test_eps_greedy_explores_in_a_tenth_of_the_rows(many_words):
    r = ar.eps_greedy(np.zeros((N_DRAWS, 5)), 0.1, *many_words)
    assert abs(r["explore"].mean() - 0.1) < 4 * math.sqrt(0.09 / N_DRAWS), r["explore"].mean()
    counts = np.bincount(r["action"][r["explore"]], minlength=5)                # uniform over the 5 actions: chi^2, 4 dof, 0.999 quantile
    exp = r["explore"].sum() / 5
    assert float(((counts - exp) ** 2 / exp).sum()) < 18.47


def test_no_row_of_the_gpu_sweep_is_ambiguous():
    """every (seed, shape, counter) tests/test_act.py draws a categorical action with: the GPU comparison leaves no row out"""
    rows = 0
    for N, A, dt, c in ar.sweep_cases():
        x = ar.logits_case(N, A, dt)
        for cc in (c, c + 1):
            r = ar.categorical(x, *ar.words(ar.SEED, cc, np.arange(N)))
            assert r["ambiguous"].sum() == 0 and not r["bad"].any(), (N, A, dt, cc)
            rows += N
    assert rows == 2 * sum(ar.NS) * len(ar.AS) * len(ar.DTYPES)
    for x, seed, c, off in ar.other_categorical_draws():      # the stream, bad-row, capture and side-stream tests
        assert ar.categorical(x, *ar.words(seed, c, np.arange(off, off + len(x))))["ambiguous"].sum() == 0, (seed, c, off)


def test_the_gaussian_cases_stay_where_tanh_is_well_conditioned():
    """|g| < 4 on every row the GPU tests draw (tests/act_restatement.py gaussian_case says why)"""
    for N in ar.NS:
        for dt in ar.DTYPES:
            for per_env in (False, True):
                mean, ls = ar.gaussian_case(N, dt, per_env)
                for c in range(8):
                    r = ar.gaussian(mean, ls, *ar.words(ar.SEED, c, np.arange(N)), squash=True)
                    assert np.abs(r["raw"]).max() < 4.0


def test_ptg_head_size_matches_the_c_compiler(tmp_path):
    import subprocess
    from rl_ptg_amd import _lib
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%zu %%zu %%zu\\n", sizeof(ptg_head), offsetof(ptg_head, in_s_n), '
                   'offsetof(ptg_head, clip_lo), offsetof(ptg_head, ent_dev));return 0;}\n' % os.path.join(ROOT, "include", "ptg_env.h"))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    H = _lib.PtgHead
    assert got == [C.sizeof(H), H.in_s_n.offset, H.clip_lo.offset, H.ent_dev.offset]


def test_the_entry_point_refuses_a_null_handle_and_the_error_code_is_minus_six():
    from rl_ptg_amd import _lib
    L = _lib.lib()
    assert L.ptg_act(None, C.byref(_lib.PtgHead()), None) == _lib.E_INVALID
    assert _lib.E_NONFINITE == -6 and L.ptg_abi_version() >= 12
    hdr = open(os.path.join(ROOT, "include", "ptg_env.h")).read()
    assert "PTG_E_NONFINITE = -6" in hdr
    assert (_lib.HEAD_CATEGORICAL, _lib.HEAD_EPS_GREEDY, _lib.HEAD_GAUSSIAN, _lib.HEAD_DETERMINISTIC, _lib.HEAD_SQUASH) == (0, 1, 2, 1, 2)


def test_python_argument_checks_need_no_device():
    import torch
    from helpers import host_engine
    eng = host_engine(6)
    x, cnt = torch.zeros(6, 5), torch.zeros(1, dtype=torch.int64)
    mean, ls = torch.zeros(6), torch.zeros(1)
    other = torch.device("meta")
    cat = lambda **kw: eng.act_categorical(kw.pop("x", x), kw.pop("cnt", cnt), **kw)
    epsg = lambda **kw: eng.act_eps_greedy(kw.pop("x", x), kw.pop("eps", 0.1), kw.pop("cnt", cnt), **kw)
    gau = lambda **kw: eng.act_gaussian(kw.pop("mean", mean), kw.pop("ls", ls), kw.pop("cnt", cnt), **kw)
    good_out = (torch.zeros(6, dtype=torch.int32), torch.zeros(6), torch.zeros(6))
    refused = [
        (TypeError, lambda: cat(x=x.half())), (TypeError, lambda: cat(x=x.numpy())), (TypeError, lambda: cat(x=x.long())),
        (ValueError, lambda: cat(x=x[:5])), (ValueError, lambda: cat(x=x[:, :1])), (ValueError, lambda: cat(x=torch.zeros(6, 33))),
        (ValueError, lambda: cat(x=torch.zeros(6))), (ValueError, lambda: cat(x=torch.zeros(5, 6).t())),          # column stride 6
        (ValueError, lambda: cat(x=torch.zeros(1, 5).expand(6, 5))),                                          # row stride 0
        (ValueError, lambda: cat(x=torch.zeros(6, 5, device=other))),
        (ValueError, lambda: cat(cnt=None)), (TypeError, lambda: cat(cnt=torch.zeros(1))), (TypeError, lambda: cat(cnt=torch.zeros(2, dtype=torch.int64))),
        (TypeError, lambda: cat(cnt=0)), (ValueError, lambda: cat(cnt=torch.zeros(1, dtype=torch.int64, device=other))),
        (TypeError, lambda: cat(act_dtype=torch.int16)), (TypeError, lambda: cat(act_dtype=torch.float32)),
        (ValueError, lambda: cat(out=good_out[:2])), (ValueError, lambda: cat(out=list(good_out))),
        (ValueError, lambda: cat(out=(good_out[0], good_out[1].double(), good_out[2]))),
        (ValueError, lambda: cat(out=(good_out[0][:5], good_out[1], good_out[2]))),
        (ValueError, lambda: cat(out=(None, good_out[1], good_out[2]))),
        (ValueError, lambda: cat(out=good_out, want_entropy=False)),                                           # an output that was not asked for
        (TypeError, lambda: cat(out=(good_out[0].short(), good_out[1], good_out[2]))),
        (ValueError, lambda: cat(out=(torch.zeros(12, dtype=torch.int32)[::2], good_out[1], good_out[2]))),
        (TypeError, lambda: epsg(eps=torch.zeros(1))), (TypeError, lambda: epsg(eps=torch.zeros(2, dtype=torch.float64))),
        (ValueError, lambda: epsg(eps=torch.zeros(1, dtype=torch.float64, device=other))), (ValueError, lambda: epsg(eps=None)),
        (ValueError, lambda: epsg(x=x[:, :1])), (ValueError, lambda: epsg(cnt=None)),
        (TypeError, lambda: gau(mean=mean.half())), (ValueError, lambda: gau(mean=torch.zeros(6, 2))), (ValueError, lambda: gau(mean=torch.zeros(5))),
        (TypeError, lambda: gau(ls=0.0)), (TypeError, lambda: gau(ls=ls.double())), (ValueError, lambda: gau(ls=torch.zeros(5))),
        (ValueError, lambda: gau(ls=torch.zeros(12)[::2])), (ValueError, lambda: gau(ls=torch.zeros(1, device=other))),
        (ValueError, lambda: gau(clip=(1.0, -1.0))), (ValueError, lambda: gau(clip=(float("nan"), 1.0))),
        (ValueError, lambda: gau(squash=True, want_entropy=True)), (ValueError, lambda: gau(cnt=None)),
        (ValueError, lambda: gau(out=(torch.zeros(6, dtype=torch.float64), None, None, None), want_raw=False, want_logp=False, want_entropy=False)),
    ]
    for k, (exc, call) in enumerate(refused):
        with pytest.raises(exc):
            call()
        assert eng._L is None, k
