"""What the GPU tests of the device rollout buffer (tests/test_rollout_buffer.py) compare against, pinned without a GPU: the NumPy
restatement of SB3's RolloutBuffer.add / reset and of the row mapping the device buffer uses (tests/rollout_buffer_restatement.py)
against a typed-out case and SB3's identities; the ctypes mirror of ptg_rollout_buffer against the C compiler; every Python-level
refusal of HipEngine.rollout_buffer_begin / rollout_buffer_add and of rl_ptg_amd.DeviceRolloutBuffer on CPU tensors, with nothing
touched and the library not reached; and what reaches the library for row-major and pitched feature-major blocks."""
import ctypes as C
import os

import numpy as np
import pytest

import gae_restatement as gr
import rollout_buffer_restatement as ro
from helpers import host_engine, recording_engine
from rl_ptg_amd.rollout_buffer import DeviceRolloutBuffer, RolloutStorage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _collect(T, N, F, rng, extra_adds=0):
    """an SB3 buffer behind collect_rollouts' lines and the device rows, fed the same T steps; returns both and the step records"""
    obs = rng.integers(0, 1 << 20, (T + 1 + extra_adds, N, F)).astype(np.float32)      # obs[k]: observation number k
    act = rng.integers(0, 5, (T + extra_adds, N)).astype(np.float32)
    val, logp, rew = (rng.standard_normal((T + extra_adds, N)).astype(np.float32) for _ in range(3))
    done = (rng.random((T + extra_adds, N)) < 0.3).astype(np.uint8)
    sb3 = ro.RolloutBuffer(T, N, F)
    col = ro.Collector(sb3, obs[0])
    dev = ro.DeviceRows(T, (N, F), np.float32, [np.float32, np.float32, np.float32, np.float32, np.uint8], N)
    dev.begin(obs[0])
    for t in range(T):
        col.collect_step(act[t], val[t], logp[t], obs[t + 1], rew[t], done[t])
        dev.add(obs[t + 1], [act[t], val[t], logp[t], rew[t], done[t]])
    return sb3, col, dev, (obs, act, val, logp, rew, done)


def test_known_answer_two_envs_three_steps():
    """T = 3, N = 2, F = 2; observation number k of env e is [100 k + 10 e, 100 k + 10 e + 1]; env 1's episode ends on step 1"""
    k, e, f = np.meshgrid(np.arange(4), np.arange(2), np.arange(2), indexing="ij")
    obs = (100 * k + 10 * e + f).astype(np.float32)
    act = np.array([[1, 2], [3, 4], [0, 1]], np.float32)
    val = np.array([[.5, .25], [1.5, 1.25], [2.5, 2.25]], np.float32)
    logp, rew = -val, 10 * val
    done = np.array([[0, 0], [0, 1], [0, 0]], np.uint8)
    sb3 = ro.RolloutBuffer(3, 2, 2)
    col = ro.Collector(sb3, obs[0])
    dev = ro.DeviceRows(3, (2, 2), np.float32, [np.float32] * 4 + [np.uint8], 2, fill=7)
    dev.begin(obs[0])
    seen = []
    for t in range(3):
        col.collect_step(act[t], val[t], logp[t], obs[t + 1], rew[t], done[t])
        dev.add(obs[t + 1], [act[t], val[t], logp[t], rew[t], done[t]])
        seen.append((sb3.pos, sb3.full, dev.pos, dev.full))
    assert seen == [(1, False, 1, False), (2, False, 2, False), (3, True, 3, True)]
    np.testing.assert_array_equal(sb3.observations[:, :, 0], [[0, 10], [100, 110], [200, 210]])            # what action t was chosen from
    np.testing.assert_array_equal(dev.rows[:, :, 1], [[1, 11], [101, 111], [201, 211], [301, 311]])         # and new_obs behind them
    np.testing.assert_array_equal(sb3.episode_starts, [[1, 1], [0, 0], [0, 1]])                             # the window opened on fresh episodes
    np.testing.assert_array_equal(dev.columns[4], [[0, 0], [0, 1], [0, 0]])
    np.testing.assert_array_equal(dev.columns[0], act)
    np.testing.assert_array_equal(sb3.actions, act)
    np.testing.assert_array_equal(col.last_obs, dev.last_obs)
    with pytest.raises(IndexError):
        sb3.add(obs[3], act[0], rew[0], done[0], val[0], logp[0])
    with pytest.raises(IndexError):
        dev.add(obs[3], [act[0], val[0], logp[0], rew[0], done[0]])
    assert dev.pos == 3
    dev.begin(dev.last_obs.copy())                          # the next window opens with the previous new_obs
    assert dev.pos == 0 and not dev.full
    np.testing.assert_array_equal(dev.rows[0], obs[3])


@pytest.mark.parametrize("T,N,F", [(1, 1, 1), (5, 3, 4), (8, 65, 2)])
def test_the_row_mapping_holds_sb3s_identities(T, N, F):
    rng = np.random.default_rng([T, N, F])
    sb3, col, dev, (obs, act, val, logp, rew, done) = _collect(T, N, F, rng)
    np.testing.assert_array_equal(dev.observations, sb3.observations)                   # observations[t] is what action t was chosen from
    np.testing.assert_array_equal(sb3.observations, obs[:T])
    np.testing.assert_array_equal(dev.last_obs, col.last_obs)                           # new_obs
    np.testing.assert_array_equal(sb3.episode_starts[1:], dev.columns[4][:-1])          # episode_starts[t + 1] == dones[t]
    np.testing.assert_array_equal(col.last_episode_starts, dev.columns[4][-1] != 0)     # the `dones` of compute_returns_and_advantage
    np.testing.assert_array_equal(ro.episode_starts_of(dev.columns[4], True), sb3.episode_starts != 0)
    for got, exp in zip(dev.columns[:4], (sb3.actions, sb3.values, sb3.log_probs, sb3.rewards)):
        np.testing.assert_array_equal(got, exp)
    # GAE on the device buffer's columns (the project's convention) == SB3's lines on SB3's own arrays
    last_values = rng.standard_normal(N).astype(np.float32)
    adv, ret = gr.gae(dev.columns[3], dev.columns[1], dev.columns[4], last_values, 0.97, 0.9, np.float32)
    with np.errstate(all="ignore"):
        adv2, ret2 = gr.compute_returns_and_advantage(sb3.rewards, sb3.values, sb3.episode_starts, last_values,
                                                      col.last_episode_starts.astype(np.float32), 0.97, 0.9)
    np.testing.assert_array_equal(adv.view(np.int32), adv2.view(np.int32))
    np.testing.assert_array_equal(ret.view(np.int32), ret2.view(np.int32))


def test_the_struct_layout_matches_the_c_compiler(tmp_path):
    import subprocess
    from rl_ptg_amd import _lib
    fs = [f for f, _ in _lib.PtgRolloutBuffer._fields_]
    assert fs == ["n_steps", "obs_dim", "obs_bytes", "obs_rows", "n_cols", "col_bytes", "col_rows", "cursor_dev"]
    body = 'printf("%zu", sizeof(ptg_rollout_buffer));\n' + "\n".join('printf(" %%zu", offsetof(ptg_rollout_buffer, %s));' % f for f in fs)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){%s return 0;}\n' % (os.path.join(ROOT, "include", "ptg_env.h"), body))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_lib.PtgRolloutBuffer)] + [getattr(_lib.PtgRolloutBuffer, f).offset for f in fs]


def test_the_entry_points_are_exported_and_refuse_a_null_handle():
    from rl_ptg_amd import _lib
    import rl_ptg_amd
    L = _lib.lib()
    d = _lib.PtgRolloutBuffer()
    assert "ptg_rollout_buffer_begin" in _lib.EXPORTS and "ptg_rollout_buffer_add" in _lib.EXPORTS
    assert L.ptg_rollout_buffer_begin(None, C.byref(d), None, 0, 0, 0, None) == _lib.E_INVALID
    assert L.ptg_rollout_buffer_add(None, C.byref(d), None, 0, 0, 0, 0, None, None, None) == _lib.E_INVALID
    assert L.ptg_abi_version() == 13
    assert rl_ptg_amd.DeviceRolloutBuffer is DeviceRolloutBuffer


def _storage(T, N, F, col_dtypes, fm=False, pitch=None):
    import torch
    pitch = N if pitch is None else pitch
    rows = torch.zeros((T + 1, F, pitch))[..., :N] if fm else torch.zeros((T + 1, N, F))
    return RolloutStorage(rows, [torch.zeros((T, N), dtype=dt) for dt in col_dtypes], torch.zeros(2, dtype=torch.int64))


def test_python_refusals_touch_nothing_and_never_reach_the_library():
    import torch
    N, T, F = 5, 3, 4
    eng = host_engine(N, obs_dim=F)
    st = _storage(T, N, F, [torch.int64, torch.float32, torch.uint8])
    obs = torch.ones((N, F))
    cols = [torch.ones(N, dtype=torch.int64), torch.ones((N, 6))[:, 5], torch.ones(N, dtype=torch.uint8)]
    gpu = torch.device("cuda", 0)
    other = host_engine(N, obs_dim=F, device=gpu)           # an engine elsewhere: every CPU tensor is on the wrong device
    add = lambda eng_=eng, **kw: eng_.rollout_buffer_add(kw.pop("st", st), kw.pop("obs", obs), kw.pop("cols", cols))
    begin = lambda **kw: eng.rollout_buffer_begin(kw.pop("st", st), kw.pop("obs", obs))
    refused = [
        (TypeError, lambda: add(obs=obs.numpy())),
        (TypeError, lambda: add(obs=obs.double())),                                      # not the rows' dtype
        (ValueError, lambda: add(obs=obs[:N - 1])),
        (ValueError, lambda: add(obs=obs[:, :F - 1])),
        (ValueError, lambda: add(obs=torch.ones((F, N)).t())),                           # [N, F], not contiguous
        (ValueError, lambda: add(obs=torch.ones((1, N, F)))),
        (ValueError, lambda: begin(obs=obs[:N - 1])),
        (TypeError, lambda: begin(obs=obs.half())),
        (ValueError, lambda: begin(obs=torch.ones((N, 2 * F))[:, :F])),
        (TypeError, lambda: add(st=st._replace(obs_rows=st.obs_rows.half()))),
        (ValueError, lambda: add(st=st._replace(obs_rows=torch.zeros((T + 1, N + 1, F))))),
        (ValueError, lambda: add(st=st._replace(obs_rows=torch.zeros((T + 1, F, N)).transpose(1, 2)))),
        (ValueError, lambda: add(st=st._replace(obs_rows=torch.zeros((1, N, F))))),      # T = 0
        (ValueError, lambda: add(st=st._replace(obs_rows=torch.zeros((N, F))))),
        (ValueError, lambda: begin(st=st._replace(obs_rows=torch.zeros((T + 1, N, 0))))),
        (ValueError, lambda: add(st=st._replace(col_rows=[st.col_rows[0]] * 9), cols=[cols[0]] * 9)),          # more than 8 columns
        (TypeError, lambda: add(st=st._replace(col_rows=[torch.zeros((T, N), dtype=torch.complex128)] + st.col_rows[1:]))),
        (ValueError, lambda: add(st=st._replace(col_rows=[st.col_rows[0][:T - 1]] + st.col_rows[1:]))),
        (ValueError, lambda: add(st=st._replace(col_rows=[torch.zeros((N, T), dtype=torch.int64).t()] + st.col_rows[1:]))),
        (TypeError, lambda: add(st=st._replace(cursor=st.cursor.float()))),
        (TypeError, lambda: add(st=st._replace(cursor=torch.zeros(3, dtype=torch.int64)))),
        (ValueError, lambda: add(st=st._replace(cursor=torch.zeros(4, dtype=torch.int64)[::2]))),
        (ValueError, lambda: add(cols=cols[:2])),                                        # a column short
        (TypeError, lambda: add(cols=[cols[0].int(), cols[1], cols[2]])),                # not the column's dtype
        (TypeError, lambda: add(cols=[cols[0], cols[1].double(), cols[2]])),
        (TypeError, lambda: add(cols=[cols[0], None, cols[2]])),
        (ValueError, lambda: add(cols=[cols[0][:N - 1], cols[1], cols[2]])),
        (ValueError, lambda: add(cols=[cols[0], torch.ones((N, 1)), cols[2]])),          # [N, 1], not [N]
        (ValueError, lambda: add(cols=[cols[0], torch.ones(N).flip(0).as_strided((N,), (0,)), cols[2]])),       # stride 0
        (ValueError, lambda: add(eng_=other)),                                           # the wrong device
    ]
    before = [t.clone() for t in (st.obs_rows, *st.col_rows, st.cursor)]
    for exc, call in refused:
        with pytest.raises(exc):
            call()
        assert eng._L is None and other._L is None
        for t, b in zip((st.obs_rows, *st.col_rows, st.cursor), before):
            assert torch.equal(t, b)
    # feature-major: the rows must have the engine's pitch
    fm = host_engine(N, obs_dim=F, feature_major=True, pitch=N + 3)
    good = _storage(T, N, F, [], fm=True, pitch=N + 3)
    block = torch.zeros((F, N + 3))[:, :N]
    for exc, call in [(ValueError, lambda: fm.rollout_buffer_begin(_storage(T, N, F, [], fm=True), block)),           # rows without the pitch
                      (ValueError, lambda: fm.rollout_buffer_begin(good, torch.zeros((F, N)))),                       # a block without it
                      (ValueError, lambda: fm.rollout_buffer_begin(good, torch.zeros((N, F)))),
                      (ValueError, lambda: fm.rollout_buffer_add(good, block, [torch.zeros(N)]))]:
        with pytest.raises(exc):
            call()
        assert fm._L is None


def test_the_buffer_class_refuses_bad_columns_before_anything_is_allocated_or_called():
    import torch
    N = 4
    eng = recording_engine(N, obs_dim=3, action_type=0)
    with pytest.raises(ValueError, match="actions"):
        DeviceRolloutBuffer(eng, 3, columns={"values": torch.float32})
    with pytest.raises(ValueError, match="kept by the buffer"):
        DeviceRolloutBuffer(eng, 3, columns={"actions": torch.int64, "rewards": torch.float32})
    with pytest.raises(ValueError, match="kept by the buffer"):
        DeviceRolloutBuffer(eng, 3, columns={"actions": torch.int64, "dones": torch.uint8})
    with pytest.raises(ValueError, match="at most 8"):
        DeviceRolloutBuffer(eng, 3, columns={"actions": torch.int64, **{f"c{k}": torch.float32 for k in range(6)}})
    with pytest.raises(ValueError, match="n_steps"):
        DeviceRolloutBuffer(eng, 0)
    buf = DeviceRolloutBuffer(eng, 3)
    assert buf.names == ["actions", "values", "log_probs", "rewards", "dones"]
    assert [buf.column(k).dtype for k in buf.names] == [torch.int64, torch.float32, torch.float32, torch.float32, torch.uint8]
    assert DeviceRolloutBuffer(recording_engine(N, obs_dim=3, action_type=1), 3).actions.dtype == torch.float32
    assert buf.observations.shape == (3, N, 3) and buf.last_obs.shape == (N, 3) and buf.advantages.shape == buf.returns.shape == (3, N)
    assert buf.observations.data_ptr() == buf.storage.obs_rows.data_ptr() and buf.last_obs.data_ptr() == buf.storage.obs_rows[3].data_ptr()
    six = DeviceRolloutBuffer(eng, 3, columns={"actions": torch.int64, **{f"c{k}": torch.float32 for k in range(5)}})
    assert len(six.names) == 8
    o, r, d = torch.zeros((N, 3)), torch.zeros(N), torch.zeros(N, dtype=torch.uint8)
    a, v = torch.zeros(N, dtype=torch.int64), torch.zeros(N)
    assert eng._L.calls == []
    for kw in (dict(actions=a, values=v), dict(actions=a, values=v, log_probs=v, entropy=v), dict(action=a, values=v, log_probs=v), {}):
        with pytest.raises(ValueError, match="differ"):
            buf.add(o, r, d, **kw)
    with pytest.raises(TypeError):
        buf.add(o, r.double(), d, actions=a, values=v, log_probs=v)
    with pytest.raises(TypeError):
        buf.add(o, r, d.float(), actions=a, values=v, log_probs=v)
    assert eng._L.calls == []
    assert (buf.cursor(), buf.pos, buf.full) == ((0, 0), 0, False)
    assert not hasattr(buf, "state_dict")
    # compute_returns_and_advantage and get say which columns they need
    bare = DeviceRolloutBuffer(eng, 3, columns={"actions": torch.int64})
    assert bare.advantages is None and bare.returns is None
    with pytest.raises(ValueError, match=r"compute_returns_and_advantage needs the columns \['values'\]"):
        bare.compute_returns_and_advantage(v, 0.99, 0.95)
    with pytest.raises(ValueError, match=r"get needs the columns \['values', 'log_probs'\].*without \['values', 'log_probs'\]"):
        next(bare.get())
    no_logp = DeviceRolloutBuffer(eng, 3, columns={"actions": torch.int64, "values": torch.float64})
    assert no_logp.advantages.dtype == no_logp.returns.dtype == torch.float64
    with pytest.raises(ValueError, match=r"without \['log_probs'\]"):
        next(no_logp.get())
    assert eng._L.calls == []


def test_what_reaches_the_library_row_major():
    import torch
    N, T, F = 6, 4, 5
    eng = recording_engine(N, obs_dim=F, action_type=0)
    eng.obs = torch.zeros((N, F))
    buf = DeviceRolloutBuffer(eng, T)
    out = torch.zeros((N, 6))                                # a joint network output: 5 logits and the value
    act, logp, rew, done = torch.zeros(N, dtype=torch.int64), torch.zeros(N), torch.zeros(N), torch.zeros(N, dtype=torch.uint8)
    new_obs = torch.zeros((N, F))
    buf.begin()
    buf.add(new_obs, rew, done, actions=act, values=out[:, 5], log_probs=logp)
    (n0, a0), (n1, a1) = eng._L.calls
    assert n0 == "ptg_rollout_buffer_begin" and n1 == "ptg_rollout_buffer_add"
    st = buf.storage
    for args, src in ((a0, eng.obs), (a1, new_obs)):
        d = args[1]._obj
        assert args[0] == "H" and args[-1] is None
        assert (d.n_steps, d.obs_dim, d.obs_bytes, d.n_cols) == (T, F, 4, 5)
        assert d.obs_rows == st.obs_rows.data_ptr() and d.cursor_dev == st.cursor.data_ptr()
        assert list(d.col_bytes)[:5] == [8, 4, 4, 4, 1] and list(d.col_rows)[:5] == [x.data_ptr() for x in st.col_rows]
        assert args[2].value == src.data_ptr()
        assert tuple(args[3:6]) == (F, 1, N * F)             # obs_s_n, obs_s_f, row_pitch
    assert len(a0) == 7 and len(a1) == 10
    assert a1[6] == 5
    assert list(a1[7])[:5] == [act.data_ptr(), out.data_ptr() + 5 * 4, logp.data_ptr(), rew.data_ptr(), done.data_ptr()]
    assert list(a1[8])[:5] == [1, 6, 1, 1, 1]                # the value column is read in place, at stride 6


def test_what_reaches_the_library_feature_major_with_a_pitch():
    import torch
    N, T, F, P = 6, 2, 5, 9
    eng = recording_engine(N, obs_dim=F, action_type=1, feature_major=True, pitch=P, out_dtype=torch.float64)
    buf = DeviceRolloutBuffer(eng, T, columns={"actions": torch.float32})
    assert buf.storage.obs_rows.shape == (T + 1, F, N) and buf.storage.obs_rows.stride() == (F * P, P, 1)
    block = eng.alloc_obs()
    buf.begin(block)
    buf.add(block, torch.zeros(N, dtype=torch.float64), torch.zeros(N, dtype=torch.uint8), actions=torch.zeros(N))
    (_, a0), (_, a1) = eng._L.calls
    for args in (a0, a1):
        d = args[1]._obj
        assert (d.n_steps, d.obs_dim, d.obs_bytes) == (T, F, 8)
        assert tuple(args[3:6]) == (1, P, F * P)
    assert a1[1]._obj.n_cols == 3 and list(a1[1]._obj.col_bytes)[:3] == [4, 8, 1] and list(a1[8])[:3] == [1, 1, 1]
    # one env: the only stride of an [N] = [1] column is free, and is passed as 1
    one = recording_engine(1, obs_dim=F, action_type=0)
    b1 = DeviceRolloutBuffer(one, T, columns={"actions": torch.int64})
    b1.add(torch.zeros((1, F)), torch.zeros(1), torch.zeros(1, dtype=torch.uint8), actions=torch.zeros((1, 3), dtype=torch.int64)[:, 0])
    assert list(one._L.calls[0][1][8])[:3] == [1, 1, 1]
