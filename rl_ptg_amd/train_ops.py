"""TrainOps: the training-side operations of the engine -- reward normalisation (vn_*), GAE, minibatch gathers (indices given or drawn on the device), the replay buffer, the
action heads, the policy loss, gSDE's matrix, head and loss, gSDE's squashed head for SAC / TQC with its backward, the TD losses, TQC's quantile loss, the training-time actor head, the actor losses, the forward and backward of the MLPs and the optimiser step.  Each method checks its tensors, marshals pointers and strides and makes one library call
(include/ptg_env.h states the arithmetic, csrc/ptg_train.hip holds the kernels, csrc/ptg_mlp.hip those of mlp_forward and mlp_backward); none of them steps the environment.  HipEngine inherits them.

The mixin reads self._torch, _L, _h, n, device, out_dtype, obs_dim, feature_major, pitch and calls self._chk, _stream, _check_obs,
_action_kind, and for split=True of the MLP ops self.consts (raw_modified, price_ahead); torch stays lazily imported (torch = self._torch).

Every tensor argument goes through ONE checker, check(), which raises in a fixed order: TypeError for what the value is (not a
tensor, a refused dtype, element size or element count), then ValueError for its shape, its strides, its device.  Nothing touches
the library and no device memory is allocated before every check of a call has passed.  Relations between arguments (old_values
iff clip_range_vf, done_col inside the columns ...) stay plain `if`s in the methods.  The blocks several ops share (_column,
_critic_columns, _alpha_arg, _out_tuple, _no_tensor_twice, _workspace_arg; TrainOps._take_workspace, _fresh_like_quantiles, _gather_args, _mlp_net,
_call) stand once, next to check(), and are called at the point of the order where each op had its own copy.  The MLP ops go one step
further: every check of one network stands once per direction (TrainOps._mlp_forward_net, _mlp_backward_net) and so does what follows the
checks (_mlp_fwd_desc, _mlp_bwd_desc); mlp_forward / mlp_backward run them once, the grouped ops once per network behind "net i:"."""
import collections
import ctypes as C

import numpy as np

from . import _lib

# what the action heads return: device tensors [N]; a field that was not asked for (or that the head does not have) is None
CategoricalAct = collections.namedtuple("CategoricalAct", "actions log_prob entropy")
EpsGreedyAct = collections.namedtuple("EpsGreedyAct", "actions")
GaussianAct = collections.namedtuple("GaussianAct", "actions raw log_prob entropy")
# what policy_loss returns: stats float64 [8], the gradients w.r.t. the head's input, the values and (Gaussian head) log_std
PolicyLoss = collections.namedtuple("PolicyLoss", "stats grad_input grad_values grad_log_std")
# what sde_act returns (GaussianAct's fields) and what sde_policy_loss returns: PolicyLoss's fields with grad_log_std [L], then the
# gradient w.r.t. the latent [B, L] (None when not asked for)
SdeAct = collections.namedtuple("SdeAct", "actions raw log_prob entropy")
SdePolicyLoss = collections.namedtuple("SdePolicyLoss", "stats grad_input grad_values grad_log_std grad_latent")
# what sde_rsample returns: actions and log_prob [B] in the inputs' dtype, step_actions float32 [B] (what step() takes), saved float64
# [B, 2] (noise, V: what sde_rsample_backward reads); sde_rsample_backward: the gradients w.r.t. the unclipped mean [B], the latent
# [B, L] and log_std [L].  Fields not asked for are None.
SdeRSample = collections.namedtuple("SdeRSample", "actions step_actions log_prob saved")
SdeRSampleGrad = collections.namedtuple("SdeRSampleGrad", "grad_mean grad_latent grad_log_std")
# what td_loss returns: stats float64 [8], the gradients w.r.t. the current Q-values (DQN: one tensor [B, A]; critics: a list of K tensors
# shaped like q[k]) and the TD target [B] (None when not asked for)
TdLoss = collections.namedtuple("TdLoss", "stats grad_q target")
# what quantile_loss returns: stats float64 [8], the gradients w.r.t. the current quantiles (a [B, K, Q] tensor or a list of K [B, Q]
# tensors, as the quantiles came) and the targets [B, M] (None when not asked for)
QuantileLoss = collections.namedtuple("QuantileLoss", "stats grad_quantiles target")
# what rsample returns: actions and log_prob shaped like mean, noise float64 (the z of every row); rsample_backward: the two gradients
RSample = collections.namedtuple("RSample", "actions log_prob noise")
RSampleGrad = collections.namedtuple("RSampleGrad", "grad_mean grad_log_std")
# what actor_loss returns: stats float64 [8], the gradients w.r.t. q (as q came; None for kind "ent_coef"), w.r.t. log_prob (None for
# "td3" / "ent_coef") and w.r.t. log alpha (float64 [1]; None without target_entropy)
ActorLoss = collections.namedtuple("ActorLoss", "stats grad_q grad_log_prob grad_log_ent_coef")
# what mlp_forward returns: out [B, O] float32; hidden: with keep_hidden the n - 1 post-activation hidden layers as [B, width_l] views into
# the workspace, else None
MlpOut = collections.namedtuple("MlpOut", "out hidden")


# what a member dict of policy_loss_group must and may name: policy_loss's arguments
_LOSS_MEMBER_NEEDS = ("head_input", "values", "actions", "old_log_prob", "advantages", "returns")
_LOSS_MEMBER_TAKES = _LOSS_MEMBER_NEEDS + ("clip_range", "clip_range_vf", "ent_coef", "vf_coef", "normalize_advantage", "old_values", "log_std", "out", "workspace")


class OptimPlan:
    """What optim_plan makes of an optimiser's tensor lists: the checked tensors (kept alive here: the device tables hold their
    addresses), the state tensors, the two device tables, the float64 device scalars and the scratch of ptg_optim_step."""
    __slots__ = ("kind", "dtype", "params", "grads", "targets", "state1", "state2", "state", "norm", "tensors_dev", "chunks_dev", "workspace",
                 "n_chunks", "grad_ptrs")


# ------------------------------------------------------------------ stride rules: None when x obeys, else what was expected
def contiguous(x):
    return None if x.is_contiguous() else "a contiguous tensor"


def rows(x):
    """[B, A] logits, possibly a column slice of a wider tensor"""
    return None if x.stride(1) == 1 and (x.shape[0] <= 1 or x.stride(0) >= x.shape[1]) else "unit column stride and a row stride >= A"


def wide_rows(x):
    """[B, L] latent rows or an exploration matrix, possibly the padded hidden layer of an MLP workspace"""
    return None if (x.shape[1] <= 1 or x.stride(1) == 1) and (x.shape[0] <= 1 or x.stride(0) >= x.shape[1]) else "unit column stride and a row stride >= L"


def step(x):
    """[B] values, possibly a column of a wider tensor"""
    return None if x.shape[0] <= 1 or x.stride(0) >= 1 else "a stride >= 1"


def one_or_all(n):
    """a parameter shared by the batch (1 element) or one per row (contiguous [n], [n, 1] or [1, n])"""
    return lambda x: None if x.numel() == 1 or (x.numel() == n and x.dim() <= 2 and x.is_contiguous()) else f"1 element or a contiguous [{n}] tensor"


def stacked(x):
    """[B, K, Q] quantiles of K critics, possibly a slice of a wider tensor: critic k is the [B, Q] view x[:, k]"""
    ok = (x.shape[2] <= 1 or x.stride(2) == 1) and x.stride(1) >= 0 and (x.shape[0] <= 1 or x.stride(0) >= x.shape[2])
    return None if ok else "unit stride along the quantiles, a row stride >= Q and a non-negative critic stride"


def non_negative(x):
    return None if min(x.stride()) >= 0 else "non-negative strides"


def strides_of(ref, dims):
    """the last `dims` strides of ref, none of them negative"""
    want = tuple(ref.stride())[-dims:]
    return lambda x: None if tuple(x.stride())[-dims:] == want and min(x.stride()) >= 0 else f"the non-negative strides {want}"


def check(eng, who, name, x, dtypes=None, sizes=None, numel=None, shape=None, rule=None, optional=False, exc=TypeError):
    """The one argument check of the training ops: x must be a tensor with one of `dtypes` or of `sizes` bytes per element and, for the
    scalar-like arguments (counter, cursor, eps, log_std), `numel` elements -- else `exc`, TypeError for inputs and ValueError for
    outputs, whose dtype is set by the inputs; then of `shape` (None entries: any size), obeying the stride `rule`, on the engine's
    device -- else ValueError.  optional: None passes.  Returns x."""
    if x is None and optional:
        return None
    if not eng._torch.is_tensor(x):
        raise exc(f"{who}: {name} must be a tensor, got {type(x).__name__}")
    if dtypes is not None and x.dtype not in dtypes:
        raise exc(f"{who}: {name} must be of {' or '.join(str(d) for d in dtypes)}, got {x.dtype}")
    if sizes is not None and x.element_size() not in sizes:
        raise exc(f"{who}: {name} must have {'-, '.join(str(s) for s in sizes)}-byte elements, got {x.dtype}")
    if numel is not None and x.numel() != numel:
        raise exc(f"{who}: {name} must have {numel} element(s), got shape {tuple(x.shape)}")
    if shape is not None:
        got = x.shape
        ok = len(got) == len(shape)
        for s, g in zip(shape, got):
            ok = ok and (s is None or s == g)
        if not ok:
            raise ValueError(f"{who}: {name} must be {['*' if s is None else s for s in shape]}, got shape {tuple(got)}")
    bad = rule(x) if rule is not None else None
    if bad:
        raise ValueError(f"{who}: {name} needs {bad}, got shape {tuple(x.shape)}, strides {tuple(x.stride())}")
    if x.device != eng.device:
        raise ValueError(f"{who}: {name} lives on {x.device}, the engine on {eng.device}")
    return x


def _dims(eng, x):
    """x.dim(); -1 for what is not a tensor, which check() then refuses"""
    return x.dim() if eng._torch.is_tensor(x) else -1


# ------------------------------------------------------------------ blocks that several ops share; each is called where the op's own text stood
def _column(eng, t):
    """[B, 1] -> [B]; anything else (None, what is no tensor) as it came, for check() to judge"""
    return t[:, 0] if _dims(eng, t) == 2 and t.shape[1] == 1 else t


def _critic_columns(eng, who, name, xs, dtypes, B=None, exc=TypeError):
    """a list of critic outputs, [B] or [B, 1] each with any stride >= 1 -> their checked [B] views; the first sets the dtype and B
    of the others"""
    cols = []
    for k, t in enumerate(xs):
        cols.append(check(eng, who, f"{name}[{k}]", _column(eng, t), dtypes=dtypes, shape=(B,), rule=step, exc=exc))
        dtypes, B = (cols[0].dtype,), cols[0].shape[0]
    return cols


def _alpha_arg(eng, who, ent_coef, log_ent_coef):
    """(alpha_dev, alpha) of a call that was given ent_coef or log_ent_coef: the checked float64 device scalar, or the Python float"""
    alpha_dev = None
    if log_ent_coef is not None or eng._torch.is_tensor(ent_coef):
        alpha_dev = check(eng, who, "log_ent_coef" if log_ent_coef is not None else "a tensor ent_coef", log_ent_coef if log_ent_coef is not None else ent_coef,
                          dtypes=(eng._torch.float64,), numel=1)
    return alpha_dev, float(ent_coef) if ent_coef is not None and alpha_dev is None else 0.0


def _out_tuple(eng, who, out, kind, stats=True):
    """out= must be a tuple as long as the namedtuple `kind`; stats: its first field is the float64 [8] statistics.  Returns out."""
    if not isinstance(out, tuple) or len(out) != len(kind._fields):
        raise ValueError(f"{who}: out must be the {kind.__name__} of an earlier call")
    if stats:
        check(eng, who, "out.stats", out[0], dtypes=(eng._torch.float64,), shape=(8,), rule=contiguous, exc=ValueError)
    return out


def _no_tensor_twice(who, tensors, what):
    """the cheap half of "outputs must not overlap": one tensor given twice"""
    starts = [t.data_ptr() for t in tensors]
    if len(set(starts)) != len(starts):
        raise ValueError(f"{who}: two of {what} start at the same address; the outputs must not overlap each other or the inputs")


def _ptr(x):
    """device pointer or NULL of a tensor; of a list of tensors, the pointer array the library takes for a column list"""
    if isinstance(x, (list, tuple)):
        return (C.c_void_p * max(len(x), 1))(*[None if t is None else t.data_ptr() for t in x])
    return None if x is None else C.c_void_p(x.data_ptr())


def _out_code(torch, dtype):
    return _lib.OUT_F64 if dtype == torch.float64 else _lib.OUT_F32


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


# ------------------------------------------------------------------ what the single and the grouped MLP ops share (TrainOps._mlp_net, _mlp_forward_net, _mlp_backward_net too)
def _pitch(w):
    """floats per row of a kept hidden layer and of a dz buffer: the width rounded up to 16 bytes (include/ptg_env.h)"""
    return (w + 3) // 4 * 4


def _row_stride(t):
    """of a [B, A] tensor; a one-row tensor may report any row stride"""
    return max(t.stride(0), t.shape[1])


def _mlp_range(who, batch, widths):
    """(batch, widths) as ints, once they lie in the range the library's *_workspace functions accept"""
    widths = [int(w) for w in widths]
    if not (1 <= int(batch) <= 2 ** 31 and 1 <= len(widths) <= _lib.MLP_MAX_LAYERS and all(1 <= w <= _lib.MLP_MAX_WIDTH for w in widths)):
        raise ValueError(f"{who}: batch must be in [1, 2^31], 1 to {_lib.MLP_MAX_LAYERS} layers, widths in [1, {_lib.MLP_MAX_WIDTH}]; got {batch}, {widths}")
    return int(batch), widths


def _workspace_arg(eng, who, label, t, need, needs="the call needs"):
    """a caller's MLP workspace -- label: its name, then in brackets the call that sizes it -- must be a contiguous uint8 tensor of
    `need` bytes or more, 4-byte aligned.  (_take_workspace asks the library for the size and knows no alignment: the loss ops' own.)"""
    name = label.split(" ")[0]
    check(eng, who, label, t, dtypes=(eng._torch.uint8,), shape=(None,), rule=contiguous, exc=ValueError)
    if t.numel() < need:
        raise ValueError(f"{who}: {name} has {t.numel()} bytes, {needs} {need}")
    if t.data_ptr() % 4:
        raise ValueError(f"{who}: {name} must be 4-byte aligned")


def _mlp_bwd_desc(eng, net, grad_out, out, workspace, grad_weights, grad_biases, grad_x, grad_x2, backward_workspace, accumulate):
    """behind the checks of a backward call: (the ptg_mlp_bwd of network `net` (what _mlp_backward_net returned) around the forward's
    descriptor, its backward workspace: the caller's, or a fresh one)"""
    torch = eng._torch
    _, widths, need, fill, _ = net
    if backward_workspace is None:
        with torch.cuda.device(eng.device):
            backward_workspace = torch.empty(need, dtype=torch.uint8, device=eng.device)
    d = _lib.PtgMlpBwd(gout_dev=_ptr(grad_out), gout_s_n=_row_stride(grad_out), dx_dev=_ptr(grad_x), dx_s_n=0 if grad_x is None else _row_stride(grad_x),
                       dx2_dev=_ptr(grad_x2), dx2_s_n=0 if grad_x2 is None else _row_stride(grad_x2), bws_dev=_ptr(backward_workspace),
                       bws_bytes=backward_workspace.numel(), flags=_lib.MLP_ACCUMULATE if accumulate else 0)
    d.fwd = fill(out, workspace, _lib.MLP_KEEP_HIDDEN)
    for l in range(len(widths)):
        if grad_weights is not None and grad_weights[l] is not None:
            d.dw_dev[l], d.dw_s_n[l], d.db_dev[l] = grad_weights[l].data_ptr(), _row_stride(grad_weights[l]), grad_biases[l].data_ptr()
    return d, backward_workspace


def _per_net(who, name, xs, G, share=False, optional=False):
    """an argument of a grouped call as a list of G entries: a list or tuple of G (ValueError for another length), with `optional` also
    None for G times None, with `share` also one tensor for all networks; TypeError for anything else"""
    if xs is None and optional:
        return [None] * G
    if isinstance(xs, (list, tuple)):
        if len(xs) != G:
            raise ValueError(f"{who}: {name} must have one entry per network, {G}, got {len(xs)}")
        return list(xs)
    if share and hasattr(xs, "data_ptr"):
        return [xs] * G
    raise TypeError(f"{who}: {name} must be a list with one entry per network{', or one tensor for all' if share else ''}{', or None' if optional else ''}, got {type(xs).__name__}")


def _mlp_fwd_desc(eng, net, out, workspace, keep_hidden, flags):
    """behind the checks of a forward call: (the ptg_mlp of network `net` (what _mlp_forward_net returned), its MlpOut, its workspace, which
    must outlive the library call), out and workspace the caller's or fresh ones; the hidden layers a keep_hidden forward leaves in its
    workspace are [B, width_l] views into it"""
    torch = eng._torch
    B, widths, need, fill = net
    if workspace is None or out is None:
        with torch.cuda.device(eng.device):
            workspace = torch.empty(need, dtype=torch.uint8, device=eng.device) if workspace is None else workspace
            out = torch.empty((B, widths[-1]), dtype=torch.float32, device=eng.device) if out is None else out
    hidden, off = [], 0
    for w in widths[:-1] if keep_hidden else ():
        p = _pitch(w)
        hidden.append(workspace[off:off + 4 * B * p].view(torch.float32).view(B, p)[:, :w])
        off += 4 * B * p
    return fill(out, workspace, flags), MlpOut(out, tuple(hidden) if keep_hidden else None), workspace


class TrainOps:
    def _call(self, name, *args):
        """one stream-ordered library call -- handle first, the current stream last -- on the engine's device, its return code checked"""
        with self._torch.cuda.device(self.device):
            self._chk(getattr(self._L, name)(self._h, *args, self._stream()))

    def _loss_workspace(self, op, batch):
        """what <op>_workspace(batch) returns: a fresh uint8 tensor of ptg_<op>_workspace(batch) bytes"""
        nbytes = getattr(self._L, f"ptg_{op}_workspace")(int(batch))
        if nbytes < 0:
            raise ValueError(f"{op}_workspace: batch must be {'>= 1' if op == 'policy_loss' else 'in [1, 2^31]'}, got {batch}")
        with self._torch.cuda.device(self.device):
            return self._torch.empty(nbytes, dtype=self._torch.uint8, device=self.device)

    def _take_workspace(self, op, B, workspace, who=None, fresh=True):
        """the workspace= of the loss `op`: the caller's, once it is a contiguous uint8 tensor of ptg_<op>_workspace(B) bytes or more,
        else a fresh one.  who: the caller's name where it is not the op's (a grouped call's "... member i"); fresh=False: only the
        check, None comes back as None"""
        who = who or op
        if workspace is None:
            return self._loss_workspace(op, B) if fresh else None
        check(self, who, f"workspace ({op}_workspace({B}))", workspace, dtypes=(self._torch.uint8,), rule=contiguous, exc=ValueError)
        size = getattr(self._L, f"ptg_{op}_workspace")
        if workspace.numel() < size(B):
            raise ValueError(f"{who}: workspace has {workspace.numel()} bytes, a batch of {B} needs {size(B)}")
        return workspace

    def _fresh_like_quantiles(self, as_list, B, K, Q, dtype):
        """fresh gradients as the quantiles came -- a list of K [B, Q] tensors or one [B, K, Q] tensor -- and their K [B, Q] views;
        called under a device guard"""
        torch = self._torch
        if as_list:
            g = [torch.empty((B, Q), dtype=dtype, device=self.device) for _ in range(K)]
            return g, g
        g = torch.empty((B, K, Q), dtype=dtype, device=self.device)
        return g, [g[:, k] for k in range(K)]

    # ------------------------------------------------------------------ VecNormalize(norm_obs=False) on the device
    def vn_init(self, gamma=0.99, epsilon=1e-8, clip_reward=10.0):
        """Start reward normalisation as the reference wraps its envs (src/rl_utils.py:453, SB3 defaults)."""
        self._chk(self._L.ptg_vn_init(self._h, float(gamma), float(epsilon), float(clip_reward)))
        self._vn_hyper = {"gamma": float(gamma), "epsilon": float(epsilon), "clip_reward": float(clip_reward)}

    def vn_normalize(self, rew, done, training=True, out=None, group=None):
        """Normalise a [T, N] (or [N]) reward tensor in place of VecNormalize.step_wait: advances the discounted returns,
        updates the running moments step by step (training=True) and returns the clipped, scaled rewards.  With an
        initialised torch.distributed process group the per-step moments of all ranks' envs are merged first (one
        all-gather per call), so every rank holds the statistics of the whole job."""
        torch = self._torch
        from . import dist as ptg_dist
        who = "vn_normalize"
        one = _dims(self, rew) == 1
        shape = (self.n,) if one else (None, self.n)
        check(self, who, "rew", rew, dtypes=(self.out_dtype,), shape=shape, rule=contiguous)      # what the kernels read
        check(self, who, "done", done, sizes=(1,), shape=rew.shape, rule=contiguous)
        check(self, who, "out", out, dtypes=(self.out_dtype,), shape=rew.shape, rule=contiguous, optional=True)
        r2, d2 = (rew.unsqueeze(0), done.unsqueeze(0)) if one else (rew, done)
        T = r2.shape[0]
        res = torch.empty_like(r2) if out is None else (out.unsqueeze(0) if one else out)
        with torch.cuda.device(self.device):
            mom = None
            if training:
                mom = torch.empty((T, 3), dtype=torch.float64, device=self.device)
                self._chk(self._L.ptg_vn_batch_moments(self._h, _ptr(r2), _ptr(d2), T, _ptr(mom), self._stream()))
                mom = ptg_dist.all_merge_moments(mom, group=group)
            self._chk(self._L.ptg_vn_apply(self._h, _ptr(r2), T, _ptr(mom), _ptr(res), 1 if training else 0, self._stream()))
            if not training:                                # frozen statistics: returns[done] = 0 all the same (SB3 step_wait)
                self._chk(self._L.ptg_vn_clear_done(self._h, _ptr(d2), T, self._stream()))
        return res[0] if one else res

    def vn_get(self):
        st, ret = np.zeros(3), np.zeros(self.n)
        self._chk(self._L.ptg_vn_get(self._h, _dp(st), _dp(ret)))
        return dict(mean=st[0], var=st[1], count=st[2]), ret

    def vn_set(self, stats=None, returns=None):
        st = None if stats is None else np.array([stats["mean"], stats["var"], stats["count"]], dtype=np.float64)
        rt = None if returns is None else np.ascontiguousarray(returns, dtype=np.float64)
        self._chk(self._L.ptg_vn_set(self._h, None if st is None else _dp(st), None if rt is None else _dp(rt)))

    # ------------------------------------------------------------------ RolloutBuffer.compute_returns_and_advantage on the device
    def gae(self, rew, values, done, last_values, gamma, gae_lambda, adv=None, ret=None):
        """Enqueue, on the current stream, the advantages and returns of a rollout in place of SB3's
        RolloutBuffer.compute_returns_and_advantage (include/ptg_env.h: ptg_gae): rew, values [T, N] (or [N] for T = 1) and
        last_values [N] of ONE float dtype (float32 or float64, whatever the engine's out_dtype), done [T, N] of a 1-byte dtype with
        rollout()'s meaning (done[t] != 0: the episode ended on step t), values[t] = V of the observation step t's action was chosen
        from, last_values = V of the observation after step T - 1.  Returns (adv, ret), allocated when not given; adv may be rew and
        ret may be values.  No synchronisation; bit for bit what NumPy computes with SB3's lines on arrays of that dtype."""
        torch = self._torch
        who = "gae"
        one = _dims(self, rew) == 1
        up = lambda x: x.unsqueeze(0) if one and _dims(self, x) == 1 else x
        r2 = check(self, who, "rew", up(rew), dtypes=(torch.float32, torch.float64), shape=(None, self.n), rule=contiguous)
        T, dt = r2.shape[0], (r2.dtype,)
        v2 = check(self, who, "values", up(values), dtypes=dt, shape=(T, self.n), rule=contiguous)
        d2 = check(self, who, "done", up(done), sizes=(1,), shape=(T, self.n), rule=contiguous)
        check(self, who, "last_values", last_values, dtypes=dt, shape=(self.n,), rule=contiguous)
        a2 = check(self, who, "adv", up(adv), dtypes=dt, shape=(T, self.n), rule=contiguous, optional=True, exc=ValueError)
        t2 = check(self, who, "ret", up(ret), dtypes=dt, shape=(T, self.n), rule=contiguous, optional=True, exc=ValueError)
        a2 = torch.empty_like(r2) if a2 is None else a2
        t2 = torch.empty_like(r2) if t2 is None else t2
        self._call("ptg_gae", _ptr(r2), _ptr(v2), _ptr(d2), _ptr(last_values), T, _out_code(torch, r2.dtype), float(gamma), float(gae_lambda), _ptr(a2), _ptr(t2))
        return (a2[0], t2[0]) if one else (a2, t2)

    # ------------------------------------------------------------------ RolloutBuffer.get on the device
    def minibatch(self, idx, obs=None, columns=(), obs_out=None, columns_out=None):
        """Enqueue, on the current stream, the gather of ONE minibatch in place of SB3's RolloutBuffer._get_samples
        (include/ptg_env.h: ptg_minibatch): idx [B] int32 / int64 sample indices in swap_and_flatten's order, i = env * T + step,
        0 <= i < T * N (slices of a torch.randperm(T * N)); obs a rollout's observation buffer as alloc_obs(T) / rollout() make it
        ([T, N, F], or [T, F, N] feature-major with the engine's pitch); columns up to 8 contiguous [T, N] tensors of 1-, 2-, 4- or
        8-byte elements (actions, values, log-probs, advantages, returns, done flags ...).  Returns (obs_out [B, F] or None,
        [column outputs [B]]), allocated when not given; row b is source row (idx[b] % T, idx[b] // T), byte for byte.  Outputs must
        not overlap inputs (not checked).  No synchronisation; an index out of range leaves its row untouched and makes the next
        sync() raise PtgError with code PTG_E_INDEX."""
        check(self, "minibatch", "idx", idx, dtypes=(self._torch.int32, self._torch.int64), shape=(None,), rule=contiguous)
        B = idx.shape[0]
        T, tail, obs_out, outs = self._gather_args("minibatch", B, obs, columns, obs_out, columns_out)
        self._call("ptg_minibatch", _ptr(idx), idx.element_size(), B, T, *tail)
        return obs_out, outs

    def _gather_args(self, who, B, obs, columns, obs_out, columns_out, rows_rule=None):
        """what minibatch and minibatch_drawn check and pass alike: (T, the library call's arguments from obs_dev on, obs_out, the
        column outputs), the outputs allocated when not given; rows_rule(T): the caller's own refusals once T is known, before
        anything is allocated"""
        torch = self._torch
        columns = list(columns)
        if obs is None and not columns:
            raise ValueError(f"{who}: neither observations nor columns given")
        if len(columns) > _lib.MB_MAX_COLS:
            raise ValueError(f"{who}: at most {_lib.MB_MAX_COLS} columns, got {len(columns)}")
        T, F, s_t, s_n, s_f = None, 0, 0, 0, 0
        if obs is not None:                                 # a [T, ...] buffer of alloc_obs(T)
            check(self, who, "obs", obs, sizes=(4, 8), shape=(None, self.obs_dim, self.n) if self.feature_major else (None, self.n, self.obs_dim),
                  rule=self._check_obs)
            T, F = obs.shape[0], self.obs_dim
            s_t, (s_n, s_f) = obs.stride(0), ((obs.stride(2), obs.stride(1)) if self.feature_major else (obs.stride(1), obs.stride(2)))
        for c, x in enumerate(columns):                     # without observations the first column sets T
            T = check(self, who, f"column {c}", x, sizes=(1, 2, 4, 8), shape=(T, self.n), rule=contiguous).shape[0]
        if columns_out is not None and len(columns_out) != len(columns):
            raise ValueError(f"{who}: {len(columns)} columns but {len(columns_out)} column outputs")
        if obs is None and obs_out is not None:
            raise ValueError(f"{who}: obs_out given without obs")
        if obs is not None:
            check(self, who, "obs_out", obs_out, dtypes=(obs.dtype,), shape=(B, F), rule=contiguous, optional=True, exc=ValueError)
        for c, (x, o) in enumerate(zip(columns, columns_out or ())):
            check(self, who, f"output of column {c}", o, dtypes=(x.dtype,), shape=(B,), rule=contiguous, exc=ValueError)
        if rows_rule is not None:
            rows_rule(T)
        with torch.cuda.device(self.device):
            if obs is not None and obs_out is None:
                obs_out = torch.empty((B, F), dtype=obs.dtype, device=self.device)
            outs = [torch.empty((B,), dtype=x.dtype, device=self.device) for x in columns] if columns_out is None else list(columns_out)
        k = len(columns)
        size = (C.c_int32 * max(k, 1))(*[x.element_size() for x in columns])
        tail = (_ptr(obs), s_t, s_n, s_f, F, obs.element_size() if obs is not None else 0, _ptr(obs_out), k, _ptr(columns), size, _ptr(outs))
        return T, tail, obs_out, outs

    def new_epoch_cursor(self):
        """The zeroed device cursor of the drawn minibatches: uint64 [2] {epochs finished, batches drawn in this epoch}, held as an
        int64 tensor.  minibatch_drawn advances it on the device, so a replayed graph draws the next batch."""
        return self._torch.zeros(2, dtype=self._torch.int64, device=self.device)

    def _epoch_cursor(self, who, cursor):
        return check(self, who, "cursor (new_epoch_cursor())", cursor, dtypes=(self._torch.int64,), numel=2, shape=(2,), rule=contiguous)

    def minibatch_drawn(self, cursor, batch_size, obs=None, columns=(), seed=0, obs_out=None, columns_out=None, idx_out=None):
        """minibatch() without a permutation in memory (include/ptg_env.h: ptg_minibatch_drawn, which states the arithmetic): the
        indices of batch cursor[1] of epoch cursor[0] are computed in the gather itself from a keyed bijection of [0, T * N) under
        (seed, epoch), and the cursor advances on the device behind it -- so ONE captured call replays through every minibatch of
        every epoch.  batch_size must divide T * N (A2C: all of it); a ragged last batch stays with minibatch().  obs, columns,
        obs_out, columns_out as in minibatch(); idx_out: int64 [B], receives the indices used.  Returns (obs_out, [column outputs],
        idx_out).  No synchronisation; with every output given, no allocation.  Not SB3's NumPy stream and not a uniform draw from
        all (T * N)! orders: a bijection whose position-to-value statistics pass for uniform at training sizes.
        Cost (profiles/minibatch_drawn_cost.txt): called eagerly it is two launches and 2.5 - 4.2 us MORE device time
        than minibatch() on a ready idx (parity had been expected and was missed at 3 of 4 shapes); what it buys is the replay -- an
        epoch of PPO gradient steps at the reference's shape took 4.0 ms as 21 replays against 16.9 ms for the eager loop over get()."""
        who = "minibatch_drawn"
        self._epoch_cursor(who, cursor)
        B = int(batch_size)
        if B < 1:
            raise ValueError(f"{who}: batch_size must be >= 1, got {batch_size}")
        check(self, who, "idx_out", idx_out, dtypes=(self._torch.int64,), shape=(B,), rule=contiguous, optional=True, exc=ValueError)

        def rows_rule(T):
            if (T * self.n) % B:
                raise ValueError(f"{who}: batch_size {B} does not divide the {T} x {self.n} rows of the rollout; a ragged last batch stays with minibatch()")
            if T * self.n > _lib.MB_DRAWN_MAX_ROWS:
                raise ValueError(f"{who}: {T} x {self.n} rows, more than 2^48")

        T, tail, obs_out, outs = self._gather_args(who, B, obs, columns, obs_out, columns_out, rows_rule)
        self._call("ptg_minibatch_drawn", _ptr(cursor), int(seed) & (2 ** 64 - 1), _ptr(idx_out), B, T, *tail)
        return obs_out, outs, idx_out

    def minibatch_end_epoch(self, cursor):
        """End an epoch that was cut short (SB3's PPO leaves its epoch loop on target_kl): the next minibatch_drawn is batch 0 of the
        next epoch.  A cursor on a fresh epoch is left alone.  One one-thread kernel on the current stream; no synchronisation."""
        self._epoch_cursor("minibatch_end_epoch", cursor)
        self._call("ptg_minibatch_end_epoch", _ptr(cursor))

    def minibatches(self, perm, batch_size, obs=None, columns=()):
        """SB3's RolloutBuffer.get loop: yields minibatch(perm[start : start + batch_size], obs, columns) for start = 0, batch_size,
        ... -- the last slice short when batch_size does not divide len(perm); batch_size None: one batch of all of perm (A2C).
        perm: a permutation of T * N on the device, e.g. torch.randperm(T * N, device=...).  Every yield has fresh outputs."""
        total = perm.shape[0]
        if batch_size is None:
            batch_size = total
        if int(batch_size) < 1:
            raise ValueError(f"minibatches: batch_size must be >= 1 or None, got {batch_size}")
        start = 0
        while start < total:
            yield self.minibatch(perm[start:start + int(batch_size)], obs, columns)
            start += int(batch_size)

    # ------------------------------------------------------------------ ReplayBuffer.add / sample on the device
    def _replay_desc(self, st, who):
        """the ptg_replay descriptor of a storage object (rl_ptg_amd.replay.ReplayStorage: obs_ring, next_ring [S, N, F], col_rings
        [S, N] each, cursor uint64-as-int64 [2]), its tensors checked"""
        torch = self._torch
        o, nx, cols, cur = st.obs_ring, st.next_ring, list(st.col_rings), st.cursor
        check(self, who, "obs_ring", o, sizes=(4, 8), shape=(None, self.n, None), rule=contiguous)
        if o.shape[0] < 1 or o.shape[2] < 1:
            raise ValueError(f"{who}: obs_ring must be [S, {self.n}, F], got shape {tuple(o.shape)}")
        check(self, who, "next_ring", nx, dtypes=(o.dtype,), shape=o.shape, rule=contiguous, exc=ValueError)
        if len(cols) > _lib.MB_MAX_COLS:
            raise ValueError(f"{who}: at most {_lib.MB_MAX_COLS} column rings, got {len(cols)}")
        for c, x in enumerate(cols):
            check(self, who, f"column ring {c}", x, sizes=(1, 2, 4, 8), shape=o.shape[:2], rule=contiguous)
        check(self, who, "cursor", cur, dtypes=(torch.int64,), numel=2, shape=(2,), rule=contiguous)
        d = _lib.PtgReplay()
        d.capacity, d.obs_dim, d.obs_bytes = o.shape[0], o.shape[2], o.element_size()
        d.obs_ring, d.next_ring, d.n_cols, d.cursor_dev = _ptr(o), _ptr(nx), len(cols), _ptr(cur)
        for c, x in enumerate(cols):
            d.col_bytes[c], d.col_ring[c] = x.element_size(), x.data_ptr()
        return d

    def replay_add(self, storage, prev_obs, obs, columns=(), done=None, final_obs=None, done_col=-1):
        """Enqueue, on the current stream, SB3's ReplayBuffer.add for a window of T vector steps (include/ptg_env.h: ptg_replay_add).
        obs is the ROW VIEW [T, N, F] of the window's observations -- rows(buffer) for a feature-major engine; any non-negative
        strides -- prev_obs [N, F] the observation the first action was chosen from and final_obs (optional, [T, N, F]) the terminal
        observations, both with obs's strides; columns one contiguous [T, N] tensor per column ring, of the ring's dtype (None at
        done_col, which is written as float32 0 / 1 from done); done [T, N] of a 1-byte dtype.  Step t goes to slot
        (cursor[0] + t) % S; the cursor advances on the device.  No synchronisation."""
        torch = self._torch
        who = "replay_add"
        d = self._replay_desc(storage, who)
        columns = list(columns)
        S, F, ring_dt = storage.obs_ring.shape[0], storage.obs_ring.shape[2], (storage.obs_ring.dtype,)
        check(self, who, "obs", obs, dtypes=ring_dt, shape=(None, self.n, F), rule=non_negative)
        T = obs.shape[0]
        if T < 1 or T > S:
            raise ValueError(f"replay_add: a window of {T} steps does not fit a buffer of {S} rows (1 <= T <= S)")
        check(self, who, "prev_obs", prev_obs, dtypes=ring_dt, shape=(self.n, F), rule=strides_of(obs, 2))
        check(self, who, "final_obs", final_obs, dtypes=ring_dt, shape=obs.shape, rule=strides_of(obs, 2 if T == 1 else 3), optional=True)
        if len(columns) != len(storage.col_rings):
            raise ValueError(f"replay_add: {len(storage.col_rings)} column rings but {len(columns)} columns")
        if not -1 <= done_col < len(columns):
            raise ValueError(f"replay_add: done_col {done_col} outside [-1, {len(columns)})")
        if done_col >= 0 and storage.col_rings[done_col].dtype != torch.float32:
            raise TypeError(f"replay_add: the done column ring must be float32, got {storage.col_rings[done_col].dtype}")
        if (done_col >= 0 or final_obs is not None) and done is None:
            raise ValueError("replay_add: final_obs and a done column need done")
        for c, x in enumerate(columns):
            if c == done_col:
                continue
            if x is None:
                raise ValueError(f"replay_add: column {c} is missing (None stands for the done column only)")
            check(self, who, f"column {c}", x, dtypes=(storage.col_rings[c].dtype,), shape=(T, self.n), rule=contiguous)
        check(self, who, "done", done, sizes=(1,), shape=(T, self.n), rule=contiguous, optional=True)
        src = _ptr([None if c == done_col else x for c, x in enumerate(columns)])
        self._call("ptg_replay_add", C.byref(d), _ptr(prev_obs), _ptr(obs), obs.stride(0), obs.stride(1), obs.stride(2), _ptr(final_obs), _ptr(done), done_col,
                   len(columns), src, T)

    def replay_sample(self, storage, batch_size=None, idx=None, seed=0, want_obs=True, want_next=True, want_cols=None, norm_col=-1,
                      want_idx=False, out=None):
        """Enqueue, on the current stream, SB3's ReplayBuffer.sample / _get_samples (include/ptg_env.h: ptg_replay_sample): a gather
        at the flat indices idx (int64 [B], i = slot * N + env) or, with idx None, at batch_size indices drawn on the device from
        (seed, cursor[1], row).  Returns (obs [B, F] | None, next_obs [B, F] | None, [column outputs [B] | None], idx_out [B] | None);
        want_cols: a bool per column ring (None: all); norm_col: the reward column, normalised as vn_normalize(training=False)
        would; out: the same 4-tuple of preallocated outputs (for a captured call).  No synchronisation; an index out of range, or a
        draw from an empty buffer, leaves its row untouched and makes the next sync() raise PtgError with code PTG_E_INDEX."""
        torch = self._torch
        who = "replay_sample"
        d = self._replay_desc(storage, who)
        k = len(storage.col_rings)
        F, ring_dt = storage.obs_ring.shape[2], storage.obs_ring.dtype
        if idx is not None:
            check(self, who, "idx", idx, dtypes=(torch.int64,), shape=(None,), rule=contiguous)
            if batch_size is not None and int(batch_size) != idx.shape[0]:
                raise ValueError(f"replay_sample: batch_size {batch_size} but {idx.shape[0]} indices")
            B = idx.shape[0]
        else:
            if batch_size is None:
                raise ValueError("replay_sample: neither idx nor batch_size given")
            B = int(batch_size)
        if B < 1:
            raise ValueError(f"replay_sample: an empty batch ({B} rows)")
        if not -1 <= norm_col < k:
            raise ValueError(f"replay_sample: norm_col {norm_col} outside [-1, {k})")
        want_cols = [True] * k if want_cols is None else [bool(w) for w in want_cols]
        if len(want_cols) != k:
            raise ValueError(f"replay_sample: {k} column rings but {len(want_cols)} entries in want_cols")
        wanted = (want_obs, want_next, want_cols, want_idx)
        if out is not None:
            o0, o1, outs, io = out
            outs = list(outs)
            if len(outs) != k:
                raise ValueError(f"replay_sample: {k} column rings but {len(outs)} column outputs")
            check(self, who, "obs output", o0, dtypes=(ring_dt,), shape=(B, F), rule=contiguous, optional=True, exc=ValueError)
            check(self, who, "next_obs output", o1, dtypes=(ring_dt,), shape=(B, F), rule=contiguous, optional=True, exc=ValueError)
            check(self, who, "idx output", io, dtypes=(torch.int64,), shape=(B,), rule=contiguous, optional=True, exc=ValueError)
            for c, (o, x) in enumerate(zip(outs, storage.col_rings)):
                check(self, who, f"output of column {c}", o, dtypes=(x.dtype,), shape=(B,), rule=contiguous, optional=True, exc=ValueError)
            wanted = (o0 is not None, o1 is not None, [o is not None for o in outs], io is not None)
        if not (wanted[0] or wanted[1] or any(wanted[2]) or wanted[3]):
            raise ValueError("replay_sample: no output asked for")
        if norm_col >= 0 and not wanted[2][norm_col]:
            raise ValueError("replay_sample: norm_col names a column without an output")
        if norm_col >= 0 and storage.col_rings[norm_col].dtype != self.out_dtype:
            raise TypeError(f"replay_sample: the reward column is {storage.col_rings[norm_col].dtype}, the engine normalises {self.out_dtype}")
        if out is None:
            with torch.cuda.device(self.device):
                mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)
                o0, o1 = mk((B, F), ring_dt) if want_obs else None, mk((B, F), ring_dt) if want_next else None
                outs = [mk((B,), x.dtype) if w else None for x, w in zip(storage.col_rings, want_cols)]
                io = mk((B,), torch.int64) if want_idx else None
        self._call("ptg_replay_sample", C.byref(d), _ptr(idx), B, int(seed) & (2 ** 64 - 1), _ptr(o0), _ptr(o1), _ptr(outs), norm_col, _ptr(io))
        return o0, o1, outs, io

    # ------------------------------------------------------------------ RolloutBuffer.reset / add on the device
    def _rollout_desc(self, st, who, obs):
        """the ptg_rollout_buffer descriptor of a storage object (rl_ptg_amd.rollout_buffer.RolloutStorage: obs_rows [T + 1, ...] as
        alloc_obs(T + 1) makes them, col_rows [T, N] each, cursor uint64-as-int64 [2]) and the (obs_s_n, obs_s_f, row_pitch) of its
        blocks; its tensors and obs, one block of the same layout, checked"""
        torch = self._torch
        rows, cols, cur = st.obs_rows, list(st.col_rows), st.cursor
        fm = self.feature_major
        check(self, who, "obs_rows", rows, sizes=(4, 8), shape=(None, None, self.n) if fm else (None, self.n, None), rule=self._check_obs)
        T, F = rows.shape[0] - 1, rows.shape[1] if fm else rows.shape[2]
        if T < 1 or F < 1:
            raise ValueError(f"{who}: obs_rows must hold T + 1 >= 2 blocks of F >= 1 features, got shape {tuple(rows.shape)}")
        if len(cols) > _lib.MB_MAX_COLS:
            raise ValueError(f"{who}: at most {_lib.MB_MAX_COLS} columns, got {len(cols)}")
        for c, x in enumerate(cols):
            check(self, who, f"col_rows {c}", x, sizes=(1, 2, 4, 8), shape=(T, self.n), rule=contiguous)
        check(self, who, "cursor", cur, dtypes=(torch.int64,), numel=2, shape=(2,), rule=contiguous)
        check(self, who, "obs", obs, dtypes=(rows.dtype,), shape=tuple(rows.shape[1:]), rule=self._check_obs)
        d = _lib.PtgRolloutBuffer()
        d.n_steps, d.obs_dim, d.obs_bytes, d.obs_rows, d.n_cols, d.cursor_dev = T, F, rows.element_size(), _ptr(rows), len(cols), _ptr(cur)
        for c, x in enumerate(cols):
            d.col_bytes[c], d.col_rows[c] = x.element_size(), x.data_ptr()
        return d, ((1, self.pitch, F * self.pitch) if fm else (F, 1, self.n * F))

    def rollout_buffer_begin(self, storage, obs):
        """Enqueue, on the current stream, SB3's RolloutBuffer.reset (include/ptg_env.h: ptg_rollout_buffer_begin): obs, an
        observation block in the engine's layout ([N, F], or [F, N] feature-major with the engine's pitch), goes to row 0 of
        storage.obs_rows and both cursor words become 0.  No synchronisation."""
        d, lay = self._rollout_desc(storage, "rollout_buffer_begin", obs)
        self._call("ptg_rollout_buffer_begin", C.byref(d), _ptr(obs), *lay)

    def rollout_buffer_add(self, storage, obs, columns=()):
        """Enqueue, on the current stream, SB3's RolloutBuffer.add for one vector step (include/ptg_env.h: ptg_rollout_buffer_add):
        with t = cursor[0] read on the device, obs -- the block step() just wrote -- goes to row t + 1 of storage.obs_rows and
        columns[c], an [N] tensor of col_rows[c]'s dtype with any stride >= 1 (a column of a wider network output is read in place),
        to col_rows[c][t]; then the cursor advances on the device, so a captured call stores at the next row on every replay.  No
        synchronisation; a call on a full buffer stores nothing and makes the next sync() raise PtgError with code PTG_E_INDEX.
        Sources must not overlap the storage (not checked)."""
        who = "rollout_buffer_add"
        d, lay = self._rollout_desc(storage, who, obs)
        columns = list(columns)
        if len(columns) != len(storage.col_rows):
            raise ValueError(f"{who}: {len(storage.col_rows)} columns in the storage but {len(columns)} given")
        for c, x in enumerate(columns):
            check(self, who, f"column {c}", x, dtypes=(storage.col_rows[c].dtype,), shape=(self.n,), rule=step)
        stride = (C.c_int64 * max(len(columns), 1))(*[x.stride(0) if self.n > 1 else 1 for x in columns])     # one env: its only stride is free
        self._call("ptg_rollout_buffer_add", C.byref(d), _ptr(obs), *lay, len(columns), _ptr(columns), stride)

    # ------------------------------------------------------------------ the action head while collecting
    def new_draw_counter(self):
        """The zeroed device counter of the action heads' draws: uint64 [1], held as an int64 tensor.  A stochastic act_* call advances
        it by one on the device, so a replayed graph draws afresh; checkpoint it with int(counter)."""
        return self._torch.zeros(1, dtype=self._torch.int64, device=self.device)

    def _act_counter(self, who, counter, deterministic):
        if counter is None and not deterministic:
            raise ValueError(f"{who}: a stochastic head needs a draw counter (new_draw_counter())")
        return check(self, who, "counter (new_draw_counter())", counter, dtypes=(self._torch.int64,), numel=1, shape=(1,), optional=True)

    def _act_outputs(self, who, kind, out, specs):
        """the output tensors of a head: out's (checked) or fresh ones; specs = [(field, wanted, dtype)] in the namedtuple's order"""
        torch = self._torch
        if out is not None:
            _out_tuple(self, who, out, kind, stats=False)
        res = []
        for k, (name, wanted, dt) in enumerate(specs):
            x = None if out is None else out[k]
            if x is not None and not wanted:
                raise ValueError(f"{who}: out.{name} given, but the head has no such output or it was not asked for")
            if out is not None and x is None and name == "actions":
                raise ValueError(f"{who}: out.actions is missing")
            res.append(check(self, who, f"out.{name}", x, dtypes=(dt,), shape=(self.n,), rule=contiguous, optional=True, exc=ValueError))
        if out is None:                                     # fresh outputs, once every given one has passed
            with torch.cuda.device(self.device):
                res = [torch.empty(self.n, dtype=dt, device=self.device) if wanted else None for _, wanted, dt in specs]
        return kind(*res)

    def _act_input(self, who, x, name, discrete):
        """logits / Q-values [N, A] with unit column stride and a row stride >= A (a slice of a wider output), or means [N] / [N, 1]"""
        torch = self._torch
        floats = (torch.float32, torch.float64)
        if discrete:
            check(self, who, name, x, dtypes=floats, shape=(self.n, None), rule=rows)
            if not 2 <= x.shape[1] <= 32:
                raise ValueError(f"{who}: {name} must be [{self.n}, A] with 2 <= A <= 32, got shape {tuple(x.shape)}")
            return x.shape[1], max(x.stride(0), x.shape[1])
        if _dims(self, x) == 2 and x.shape[1] == 1:                         # [N, 1]: the env's Box has one dimension
            x = x[:, 0]
        check(self, who, name, x, dtypes=floats, shape=(self.n,), rule=step)
        return 1, max(x.stride(0), 1)

    def _act_dtype(self, who, act_dtype, out):
        """the discrete heads' action dtype: the caller's, else that of out.actions, else int32"""
        torch = self._torch
        if act_dtype is None and isinstance(out, tuple) and out and torch.is_tensor(out[0]):
            act_dtype = out[0].dtype
        act_dtype = torch.int32 if act_dtype is None else act_dtype
        if act_dtype not in (torch.int32, torch.int64):
            raise TypeError(f"{who}: act_dtype must be torch.int32 or torch.int64, got {act_dtype}")
        return act_dtype

    def _act_launch(self, head, x, counter, seed, res):
        torch = self._torch
        head.in_dtype = _out_code(torch, x.dtype)
        head.in_dev, head.seed, head.counter_dev = _ptr(x), int(seed) & (2 ** 64 - 1), _ptr(counter)
        head.act_dev, head.logp_dev, head.ent_dev = _ptr(res.actions), _ptr(getattr(res, "log_prob", None)), _ptr(getattr(res, "entropy", None))
        head.raw_dev = _ptr(getattr(res, "raw", None))
        head.act_kind = self._action_kind(res.actions)
        self._call("ptg_act", C.byref(head))
        return res

    def act_categorical(self, logits, counter, seed=0, deterministic=False, out=None, want_logp=True, want_entropy=True, act_dtype=None):
        """Enqueue, on the current stream, SB3's CategoricalDistribution.sample (deterministic: mode), log_prob and entropy of the
        logits [N, A] (float32 / float64, 2 <= A <= 32, a column slice of a wider tensor is fine) in ONE launch (include/ptg_env.h:
        ptg_act, which states the arithmetic).  act_dtype None: the dtype of out.actions when out is given, else torch.int32 (torch is
        imported lazily here, so the default is spelled None).  counter: new_draw_counter(); row e of the c-th call draws from (seed, c, global env
        offset + e).  Returns CategoricalAct(actions [N] of act_dtype (torch.int32, the default, or int64: what step() takes), log_prob
        [N], entropy [N] in the logits' dtype, or None when not wanted); out: an earlier call's result, reused (a captured call).
        No synchronisation; a row with a NaN or +Inf logit, or -Inf in every column, gets action 0 and NaN outputs and makes the next
        sync() raise PtgError with code PTG_E_NONFINITE."""
        who = "act_categorical"
        A, s_n = self._act_input(who, logits, "logits", True)
        counter = self._act_counter(who, counter, deterministic)
        res = self._act_outputs(who, CategoricalAct, out, [("actions", True, self._act_dtype(who, act_dtype, out)), ("log_prob", want_logp, logits.dtype),
                                                           ("entropy", want_entropy, logits.dtype)])
        head = _lib.PtgHead(kind=_lib.HEAD_CATEGORICAL, flags=_lib.HEAD_DETERMINISTIC if deterministic else 0, n_actions=A, in_s_n=s_n)
        return self._act_launch(head, logits, counter, seed, res)

    def act_eps_greedy(self, q, eps, counter, seed=0, deterministic=False, out=None, act_dtype=None):
        """DQN's collecting policy in one launch: with probability eps a uniform random action, else the first maximal Q-value of
        q [N, A]; deterministic: always the latter (eps is not read).  eps: a float64 device tensor of 1 element, read when the kernel
        runs (anneal it in place between replays), or a Python float, written to a fresh device scalar by a fill kernel ahead of the head
        on the same stream -- a captured call then keeps that value on every replay.
        Returns EpsGreedyAct(actions).  A row with a NaN or +Inf value, and every row when eps is NaN or outside [0, 1], gets action 0
        and makes the next sync() raise PtgError with code PTG_E_NONFINITE."""
        torch = self._torch
        who = "act_eps_greedy"
        A, s_n = self._act_input(who, q, "q", True)
        counter = self._act_counter(who, counter, deterministic)
        if torch.is_tensor(eps):
            check(self, who, "a tensor eps", eps, dtypes=(torch.float64,), numel=1)
        elif eps is None:
            if not deterministic:
                raise ValueError(f"{who}: a stochastic call needs eps")
        else:
            eps = float(eps)                                  # written to the device below, once every check has passed
        res = self._act_outputs(who, EpsGreedyAct, out, [("actions", True, self._act_dtype(who, act_dtype, out))])
        if isinstance(eps, float):                            # a fill kernel on the current stream, not a host copy: it can be captured, and
            with torch.cuda.device(self.device):              # a replay then writes the same value into the graph's own memory
                eps = torch.full((1,), eps, dtype=torch.float64, device=self.device)
        head = _lib.PtgHead(kind=_lib.HEAD_EPS_GREEDY, flags=_lib.HEAD_DETERMINISTIC if deterministic else 0, n_actions=A, in_s_n=s_n,
                            param_dev=_ptr(eps))
        return self._act_launch(head, q, counter, seed, res)

    def act_gaussian(self, mean, log_std, counter, clip=(-1.0, 1.0), squash=False, seed=0, deterministic=False, out=None, want_raw=True,
                     want_logp=True, want_entropy=None):
        """The Gaussian heads in one launch: g = mean + exp(log_std) * z, z a Box-Muller normal (deterministic: z = 0).  Plain
        (TD3 with log_std = log(sigma_exp); continuous A2C / PPO): actions = clip(g), log_prob and entropy of N(mean, sigma);
        squash=True (SAC / TQC): actions = clip(tanh(g)), log_prob with SB3's tanh correction, no entropy.  mean [N] (or [N, 1]),
        log_std of mean's dtype: 1 element (state-independent) or [N]; both may be rewritten between replays.  Returns
        GaussianAct(actions float32 [N] for step(), raw = g unclipped and unsquashed (what an on-policy buffer stores), log_prob,
        entropy).  A non-finite mean or a NaN / +Inf log_std gives action 0, NaN outputs and PTG_E_NONFINITE at the next sync()."""
        torch = self._torch
        who = "act_gaussian"
        _, s_n = self._act_input(who, mean, "mean", False)
        m1 = mean[:, 0] if mean.dim() == 2 else mean
        check(self, who, "log_std", log_std, dtypes=(mean.dtype,), rule=one_or_all(self.n))
        lo, hi = float(clip[0]), float(clip[1])
        if not lo <= hi:
            raise ValueError(f"{who}: clip {clip} is not an interval")
        if want_entropy is None:
            want_entropy = not squash
        if squash and want_entropy:
            raise ValueError(f"{who}: a squashed Gaussian has no closed-form entropy")
        counter = self._act_counter(who, counter, deterministic)
        res = self._act_outputs(who, GaussianAct, out, [("actions", True, torch.float32), ("raw", want_raw, mean.dtype), ("log_prob", want_logp, mean.dtype),
                                                        ("entropy", want_entropy, mean.dtype)])
        flags = (_lib.HEAD_DETERMINISTIC if deterministic else 0) | (_lib.HEAD_SQUASH if squash else 0)
        head = _lib.PtgHead(kind=_lib.HEAD_GAUSSIAN, flags=flags, in_s_n=s_n, param_dev=_ptr(log_std), param_s_n=0 if log_std.numel() == 1 else 1,
                            clip_lo=lo, clip_hi=hi)
        return self._act_launch(head, m1, counter, seed, res)

    # ------------------------------------------------------------------ the loss of a minibatch and its gradients
    def policy_loss_workspace(self, batch):
        """the device scratch of policy_loss for a batch of this size (a uint8 tensor; reuse it across calls of up to that size)"""
        return self._loss_workspace("policy_loss", batch)

    def policy_loss(self, kind, head_input, values, actions, old_log_prob, advantages, returns, *, clip_range=None, clip_range_vf=None,
                    ent_coef=0.0, vf_coef=0.5, normalize_advantage=None, old_values=None, log_std=None, out=None, workspace=None):
        """Enqueue, on the current stream, SB3's evaluate_actions and the loss lines of PPO.train (kind "ppo") or A2C.train ("a2c") on
        one minibatch together with their gradients (include/ptg_env.h: ptg_policy_loss, which states the arithmetic).
        head_input: logits [B, A] (2 <= A <= 32, unit column stride, row stride >= A: a column slice of an [B, A + 1] actor-critic
        output is fine) with int32 / int64 actions [B] -- or, with log_std (a 1-element tensor), the Gaussian head's means [B] /
        [B, 1] with the stored raw samples [B] as actions.  values [B] (any stride >= 1); old_log_prob (PPO; None for A2C),
        advantages, returns and old_values (required iff clip_range_vf is given) contiguous [B]; every float tensor of ONE dtype,
        float32 or float64.  clip_range is required for PPO.  normalize_advantage None: SB3's default, True for PPO, False for A2C.
        Returns PolicyLoss(stats float64 [8] = loss, policy_loss, value_loss, entropy_loss, approx_kl, clip_fraction, adv mean, adv
        std; grad_input = d loss / d head_input, shaped like it; grad_values [B]; grad_log_std [1] or None).  out: an earlier result
        (or any such tuple: grad_input and grad_values may be views of one [B, A + 1] tensor), reused by a captured call; workspace:
        policy_loss_workspace(B) or larger, allocated when missing.  Fresh gradients are torch.empty: a row refused for its action
        keeps what was there.  No synchronisation; a bad row makes the next sync() raise PtgError (PTG_E_INDEX / PTG_E_NONFINITE)."""
        d, res, _ = self._policy_loss_member("policy_loss", kind, head_input, values, actions, old_log_prob, advantages, returns, clip_range=clip_range,
                                             clip_range_vf=clip_range_vf, ent_coef=ent_coef, vf_coef=vf_coef, normalize_advantage=normalize_advantage,
                                             old_values=old_values, log_std=log_std, out=out, workspace=workspace)[1]()
        self._call("ptg_policy_loss", C.byref(d))
        return res

    def _policy_loss_member(self, who, kind, head_input, values, actions, old_log_prob, advantages, returns, *, clip_range=None, clip_range_vf=None,
                            ent_coef=0.0, vf_coef=0.5, normalize_advantage=None, old_values=None, log_std=None, out=None, workspace=None):
        """Every check of ONE policy-loss call, in policy_loss's order, for policy_loss and for each member of policy_loss_group (who:
        "policy_loss", or "policy_loss_group: member i").  Allocates nothing and does not touch the library.  Returns (what a group
        must agree in, as (name, value) pairs; make; the outputs and workspace the caller gave), where make() allocates what was not
        given and returns (the PtgLoss, the PolicyLoss, the workspace, which must outlive the library call)."""
        torch = self._torch
        if kind not in ("ppo", "a2c"):
            raise ValueError(f"{who}: kind must be 'ppo' or 'a2c', got {kind!r}")
        ppo, gauss = kind == "ppo", log_std is not None
        if gauss:                                           # the means [B] or [B, 1]
            x = check(self, who, "head_input (the means, with log_std)", _column(self, head_input), dtypes=(torch.float32, torch.float64), shape=(None,), rule=step)
            (B,), A = x.shape, 0
        else:
            x = check(self, who, "head_input (logits; or means with log_std)", head_input, dtypes=(torch.float32, torch.float64), shape=(None, None), rule=rows)
            B, A = x.shape
            if not 2 <= A <= 32:
                raise ValueError(f"{who}: head_input must be logits [B, A] with 2 <= A <= 32 (or means [B] with log_std), got shape {tuple(x.shape)}")
        if B < 1:
            raise ValueError(f"{who}: an empty batch, head_input has shape {tuple(head_input.shape)}")
        dt = (x.dtype,)
        check(self, who, "log_std", log_std, dtypes=dt, numel=1, optional=True)
        values = check(self, who, "values", _column(self, values), dtypes=dt, shape=(B,), rule=step)
        if clip_range_vf is not None and old_values is None:
            raise ValueError(f"{who}: clip_range_vf needs old_values")
        if ppo and old_log_prob is None:
            raise ValueError(f"{who}: PPO needs old_log_prob")
        check(self, who, "actions (the raw samples)" if gauss else "actions", actions, dtypes=dt if gauss else (torch.int32, torch.int64), shape=(B,), rule=contiguous)
        cols = [("advantages", advantages), ("returns", returns)] + ([("old_log_prob", old_log_prob)] if ppo else [])
        for name, c in cols + ([("old_values", old_values)] if clip_range_vf is not None else []):
            check(self, who, name, c, dtypes=dt, shape=(B,), rule=contiguous)
        if ppo:
            if clip_range is None or not float(clip_range) >= 0.0:
                raise ValueError(f"{who}: PPO needs a clip_range >= 0, got {clip_range}")
        if clip_range_vf is not None and not float(clip_range_vf) >= 0.0:
            raise ValueError(f"{who}: clip_range_vf must be >= 0 (or None), got {clip_range_vf}")
        if normalize_advantage is None:
            normalize_advantage = ppo
        if out is not None:
            stats, g_in, g_val, g_ls = _out_tuple(self, who, out, PolicyLoss, stats=False)
            if not gauss and g_ls is not None:
                raise ValueError(f"{who}: out.grad_log_std given, but the categorical head has no log_std")
            check(self, who, "out.stats", stats, dtypes=(torch.float64,), shape=(8,), rule=contiguous, exc=ValueError)
            g_in = check(self, who, "out.grad_input", _column(self, g_in) if gauss else g_in, dtypes=dt, shape=x.shape, rule=step if gauss else rows, exc=ValueError)
            check(self, who, "out.grad_values", g_val, dtypes=dt, shape=(B,), rule=step, exc=ValueError)
            if gauss:
                check(self, who, "out.grad_log_std", g_ls, dtypes=dt, shape=(1,), exc=ValueError)
        self._take_workspace("policy_loss", B, workspace, who=who, fresh=False)
        agree = (("kind", kind), ("the head", "gaussian" if gauss else "categorical"), ("normalize_advantage", bool(normalize_advantage)),
                 ("clip_range_vf given or not", clip_range_vf is not None), ("the number of actions", A), ("the dtype", x.dtype),
                 ("the actions' dtype", actions.dtype), ("the batch", B))
        given = ([] if out is None else [stats, g_in, g_val]) + ([] if workspace is None else [workspace])

        def make():
            return self._policy_loss_desc(kind, x, values, actions, old_log_prob, advantages, returns, clip_range, clip_range_vf, ent_coef, vf_coef, normalize_advantage,
                                          old_values, log_std, None if out is None else (stats, g_in, g_val, g_ls), workspace)
        return agree, make, given

    def _policy_loss_desc(self, kind, x, values, actions, old_log_prob, advantages, returns, clip_range, clip_range_vf, ent_coef, vf_coef, normalize_advantage,
                          old_values, log_std, out, workspace):
        """behind the checks of _policy_loss_member: (the PtgLoss, the PolicyLoss, the workspace), outputs and workspace the caller's or fresh"""
        torch = self._torch
        ppo, gauss = kind == "ppo", log_std is not None
        B, A = x.shape[0], 0 if gauss else x.shape[1]
        if workspace is None:
            workspace = self._loss_workspace("policy_loss", B)
        if out is None:
            with torch.cuda.device(self.device):
                stats = torch.empty(8, dtype=torch.float64, device=self.device)
                g_in = torch.empty(tuple(x.shape), dtype=x.dtype, device=self.device)
                g_val = torch.empty(B, dtype=x.dtype, device=self.device)
                g_ls = torch.empty(1, dtype=x.dtype, device=self.device) if gauss else None
        else:
            stats, g_in, g_val, g_ls = out
        d = _lib.PtgLoss(kind=_lib.LOSS_PPO if ppo else _lib.LOSS_A2C, head=_lib.HEAD_GAUSSIAN if gauss else _lib.HEAD_CATEGORICAL,
                         flags=(_lib.LOSS_NORM_ADV if normalize_advantage else 0) | (_lib.LOSS_CLIP_VF if clip_range_vf is not None else 0),
                         n_actions=A, in_dtype=_out_code(torch, x.dtype), act_kind=_lib.ACT_I64 if actions.dtype == torch.int64 else _lib.ACT_I32,
                         batch=B, in_dev=_ptr(x), in_s_n=max(x.stride(0), A, 1), val_dev=_ptr(values), val_s_n=max(values.stride(0), 1),
                         act_dev=_ptr(actions), old_logp_dev=_ptr(old_log_prob if ppo else None), adv_dev=_ptr(advantages), ret_dev=_ptr(returns),
                         old_val_dev=_ptr(old_values if clip_range_vf is not None else None), log_std_dev=_ptr(log_std),
                         clip_range=float(clip_range) if ppo else 0.0, clip_range_vf=float(clip_range_vf) if clip_range_vf is not None else 0.0,
                         ent_coef=float(ent_coef), vf_coef=float(vf_coef), stats_dev=_ptr(stats), grad_in_dev=_ptr(g_in),
                         g_s_n=max(g_in.stride(0), A, 1), grad_val_dev=_ptr(g_val), gv_s_n=max(g_val.stride(0), 1),
                         grad_log_std_dev=_ptr(g_ls if gauss else None), ws_dev=_ptr(workspace))
        return d, PolicyLoss(stats, g_in, g_val, g_ls), workspace

    def policy_loss_group(self, kind, members, *, clip_range=None, clip_range_vf=None, ent_coef=0.0, vf_coef=0.5, normalize_advantage=None):
        """policy_loss for G independent minibatches of ONE batch size, 1 <= G <= 8, in exactly the launches of one policy_loss call
        (include/ptg_env.h: ptg_policy_loss_group): the agents of a seed sweep.  Every member's result is, bit
        for bit, what policy_loss gives for its arguments.  members: a list of G dicts of policy_loss's arguments by name (head_input,
        values, actions, old_log_prob, advantages, returns, and any of clip_range, clip_range_vf, ent_coef, vf_coef, old_values, log_std,
        out, workspace); the keyword arguments here are the defaults of the members that do not name them.  The members must agree in
        kind, head, normalize_advantage, whether clip_range_vf is given, A, the dtypes and B (ValueError, which names the two members);
        every scalar may differ.  No tensor may serve two members as an output or workspace.  Checked as policy_loss checks, member by
        member, the message behind "member i:"; the library is not touched and nothing is allocated before every check has passed, and
        nothing at all when every member brings out= and workspace=.  Returns the list of G PolicyLoss.
        Cost (profiles/train_group_cost.txt; DESIGN.md section 26, whose one condition held at every shape): see DeviceOptimizerGroup's docstring."""
        who = "policy_loss_group"
        if not isinstance(members, (list, tuple)) or not all(isinstance(m, dict) for m in members):
            raise TypeError(f"{who}: members must be a list of dicts of policy_loss's arguments, got {type(members).__name__}")
        G = len(members)
        if not 1 <= G <= _lib.TRAIN_GROUP_MAX:
            raise ValueError(f"{who}: 1 to {_lib.TRAIN_GROUP_MAX} members, got {G}")
        shared = dict(clip_range=clip_range, clip_range_vf=clip_range_vf, ent_coef=ent_coef, vf_coef=vf_coef, normalize_advantage=normalize_advantage)
        checked = []
        for i, m in enumerate(members):
            kw = dict(shared, **m)
            if kind == "a2c":
                kw.setdefault("old_log_prob", None)
            missing, unknown = [k for k in _LOSS_MEMBER_NEEDS if k not in kw], [k for k in kw if k not in _LOSS_MEMBER_TAKES]
            if missing or unknown:
                raise TypeError(f"{who}: member {i}: a member names policy_loss's arguments; missing {missing}, unknown {unknown}")
            checked.append(self._policy_loss_member(f"{who}: member {i}", kind, **kw))
        for i, (agree, _, _) in enumerate(checked):
            for (name, a), (_, b) in zip(checked[0][0], agree):
                if a != b:
                    raise ValueError(f"{who}: members 0 and {i} disagree in {name}: {a} and {b}")
        _no_tensor_twice(who, [t for _, _, given in checked for t in given], "the members' outputs and workspaces")
        made = [make() for _, make, _ in checked]
        self._call("ptg_policy_loss_group", (_lib.PtgLoss * G)(*[m[0] for m in made]), G)      # made holds the workspaces until here
        return [m[1] for m in made]

    # ------------------------------------------------------------------ gSDE: the exploration matrix, the collecting head, its loss
    def _sde_log_std(self, who, log_std, dtypes, L=None):
        """log_std [L] or [L, 1] contiguous (SB3's parameter with the env's one action dimension) -> (the checked tensor, L)"""
        if _dims(self, log_std) == 2 and log_std.shape[1] == 1:
            log_std = log_std[:, 0]
        check(self, who, "log_std", log_std, dtypes=dtypes, shape=(L,), rule=contiguous)
        if not 1 <= log_std.shape[0] <= _lib.MLP_MAX_WIDTH:
            raise ValueError(f"{who}: log_std must have 1 to {_lib.MLP_MAX_WIDTH} entries, got shape {tuple(log_std.shape)}")
        return log_std, log_std.shape[0]

    def sde_resample(self, log_std, counter, noise, seed=0):
        """Enqueue SB3's StateDependentNoiseDistribution.sample_weights on the current stream (include/ptg_env.h: ptg_sde_resample):
        noise [N, L] (log_std's dtype, unit column stride, row stride >= L) is filled with exp(log_std[k]) * z, z the draw of
        (seed, *counter, (global env offset + e) * 1024 + k); counter: new_draw_counter(), advanced by one on the device.  log_std [L]
        or [L, 1], float32 or float64, read when the kernel runs.  Returns noise.  A NaN or +Inf log_std entry makes its column NaN and
        the next sync() raise PtgError with code PTG_E_NONFINITE."""
        torch = self._torch
        who = "sde_resample"
        log_std, L = self._sde_log_std(who, log_std, (torch.float32, torch.float64))
        check(self, who, "counter (new_draw_counter())", counter, dtypes=(torch.int64,), numel=1, shape=(1,))
        check(self, who, "noise", noise, dtypes=(log_std.dtype,), shape=(self.n, L), rule=wide_rows, exc=ValueError)
        d = _lib.PtgSdeNoise(in_dtype=_out_code(torch, log_std.dtype), latent_dim=L, log_std_dev=_ptr(log_std), seed=int(seed) & (2 ** 64 - 1),
                             counter_dev=_ptr(counter), e_dev=_ptr(noise), e_s_n=_row_stride(noise))
        self._call("ptg_sde_resample", C.byref(d))
        return noise

    def sde_act_outputs(self, dtype):
        """fresh outputs of sde_act for its out=: what a captured collect step writes on every replay"""
        torch = self._torch
        with torch.cuda.device(self.device):
            return SdeAct(torch.zeros(self.n, dtype=torch.float32, device=self.device), *[torch.zeros(self.n, dtype=dtype, device=self.device) for _ in range(3)])

    def sde_act(self, mean, latent, log_std, noise, clip=(-1.0, 1.0), deterministic=False, out=None, want_raw=True, want_logp=True, want_entropy=True):
        """gSDE's collecting head in one launch (include/ptg_env.h: ptg_sde_act): g = mean + latent . noise row by row, the variance
        (latent^2) . exp(log_std)^2 + 1e-6; deterministic: g = mean and noise may be None.  mean [N] / [N, 1] (any stride >= 1),
        latent [N, L] and noise [N, L] (unit column stride, row stride >= L: the kept hidden layer of an MLP forward is taken in place),
        log_std [L] / [L, 1], all of ONE dtype, float32 or float64.  Returns SdeAct(actions float32 [N] clipped for step(), raw = g (what
        an on-policy buffer stores), log_prob, entropy).  A non-finite mean or latent entry, or a NaN / +Inf log_std, gives action 0,
        NaN outputs and PTG_E_NONFINITE at the next sync()."""
        torch = self._torch
        who = "sde_act"
        _, s_n = self._act_input(who, mean, "mean", False)
        m1 = mean[:, 0] if mean.dim() == 2 else mean
        dt = (mean.dtype,)
        log_std, L = self._sde_log_std(who, log_std, dt)
        check(self, who, "latent", latent, dtypes=dt, shape=(self.n, L), rule=wide_rows)
        if noise is None and not deterministic:
            raise ValueError(f"{who}: a stochastic head needs the exploration matrix (sde_resample)")
        check(self, who, "noise", noise, dtypes=dt, shape=(self.n, L), rule=wide_rows, optional=True)
        lo, hi = float(clip[0]), float(clip[1])
        if not lo <= hi:
            raise ValueError(f"{who}: clip {clip} is not an interval")
        res = self._act_outputs(who, SdeAct, out, [("actions", True, torch.float32), ("raw", want_raw, mean.dtype), ("log_prob", want_logp, mean.dtype),
                                                   ("entropy", want_entropy, mean.dtype)])
        stochastic = not deterministic
        d = _lib.PtgSdeHead(flags=_lib.HEAD_DETERMINISTIC if deterministic else 0, in_dtype=_out_code(torch, mean.dtype), latent_dim=L,
                            act_kind=_lib.ACT_F32, mean_dev=_ptr(m1), mean_s_n=s_n, latent_dev=_ptr(latent), latent_s_n=_row_stride(latent),
                            e_dev=_ptr(noise if stochastic else None), e_s_n=_row_stride(noise) if stochastic else 0, log_std_dev=_ptr(log_std),
                            clip_lo=lo, clip_hi=hi, act_dev=_ptr(res.actions), raw_dev=_ptr(res.raw), logp_dev=_ptr(res.log_prob), ent_dev=_ptr(res.entropy))
        self._call("ptg_sde_act", C.byref(d))
        return res

    @staticmethod
    def sde_policy_loss_workspace_bytes(batch, latent_dim):
        """ptg_sde_policy_loss_workspace restated: 8 * (4 + 3 m + L + n * (8 + L)) with m blocks of 256 rows for the advantage moments
        and n blocks of 4 * ceil(B / 4096) rows for the row kernel; -1 outside the ranges the library accepts"""
        B, L = int(batch), int(latent_dim)
        if not (1 <= B <= 2 ** 31 and 1 <= L <= _lib.MLP_MAX_WIDTH):
            return -1
        per = 4 * ((B - 1) // 4096 + 1)
        return 8 * (4 + 3 * ((B - 1) // 256 + 1) + L + ((B - 1) // per + 1) * (8 + L))

    def sde_policy_loss_workspace(self, batch, latent_dim):
        """the device scratch of sde_policy_loss for a batch of this size and latent width (a uint8 tensor)"""
        nbytes = self._L.ptg_sde_policy_loss_workspace(int(batch), int(latent_dim))
        if nbytes < 0:
            raise ValueError(f"sde_policy_loss_workspace: batch must be in [1, 2^31] and latent_dim in [1, {_lib.MLP_MAX_WIDTH}], got {batch}, {latent_dim}")
        with self._torch.cuda.device(self.device):
            return self._torch.empty(nbytes, dtype=self._torch.uint8, device=self.device)

    def sde_policy_loss(self, kind, mean, values, latent, log_std, actions, old_log_prob, advantages, returns, *, clip_range=None, clip_range_vf=None,
                        ent_coef=0.0, vf_coef=0.5, normalize_advantage=None, old_values=None, want_grad_latent=False, out=None, workspace=None):
        """policy_loss for gSDE's head (include/ptg_env.h: ptg_sde_policy_loss): SB3's evaluate_actions on
        StateDependentNoiseDistribution and the loss lines of PPO.train ("ppo") / A2C.train ("a2c") with their gradients.  mean [B] /
        [B, 1] and values [B] (any stride >= 1), latent [B, L] (unit column stride, row stride >= L), log_std [L] / [L, 1], actions [B]
        the stored raw samples; the other arguments as policy_loss takes them; every float tensor of ONE dtype.  Returns
        SdePolicyLoss(stats float64 [8] as policy_loss gives them, grad_input = d loss / d mean shaped like mean, grad_values [B],
        grad_log_std [L], grad_latent [B, L] with want_grad_latent (SB3's learn_features=True) else None).  out: an earlier result,
        reused by a captured call (its grad_latent decides whether that gradient is written); workspace:
        sde_policy_loss_workspace(B, L) or larger.  No synchronisation; a bad row makes the next sync() raise PtgError."""
        torch = self._torch
        who = "sde_policy_loss"
        if kind not in ("ppo", "a2c"):
            raise ValueError(f"{who}: kind must be 'ppo' or 'a2c', got {kind!r}")
        ppo = kind == "ppo"
        x = check(self, who, "mean", _column(self, mean), dtypes=(torch.float32, torch.float64), shape=(None,), rule=step)
        (B,) = x.shape
        if B < 1:
            raise ValueError(f"{who}: an empty batch, mean has shape {tuple(mean.shape)}")
        dt = (x.dtype,)
        log_std, L = self._sde_log_std(who, log_std, dt)
        check(self, who, "latent", latent, dtypes=dt, shape=(B, L), rule=wide_rows)
        values = check(self, who, "values", _column(self, values), dtypes=dt, shape=(B,), rule=step)
        if clip_range_vf is not None and old_values is None:
            raise ValueError(f"{who}: clip_range_vf needs old_values")
        if ppo and old_log_prob is None:
            raise ValueError(f"{who}: PPO needs old_log_prob")
        cols = [("actions (the raw samples)", actions), ("advantages", advantages), ("returns", returns)] + ([("old_log_prob", old_log_prob)] if ppo else [])
        for name, c in cols + ([("old_values", old_values)] if clip_range_vf is not None else []):
            check(self, who, name, c, dtypes=dt, shape=(B,), rule=contiguous)
        if ppo:
            if clip_range is None or not float(clip_range) >= 0.0:
                raise ValueError(f"{who}: PPO needs a clip_range >= 0, got {clip_range}")
        if clip_range_vf is not None and not float(clip_range_vf) >= 0.0:
            raise ValueError(f"{who}: clip_range_vf must be >= 0 (or None), got {clip_range_vf}")
        if normalize_advantage is None:
            normalize_advantage = ppo
        if out is not None:
            stats, g_in, g_val, g_ls, g_lat = _out_tuple(self, who, out, SdePolicyLoss)
            g_in = check(self, who, "out.grad_input", _column(self, g_in), dtypes=dt, shape=(B,), rule=step, exc=ValueError)
            check(self, who, "out.grad_values", g_val, dtypes=dt, shape=(B,), rule=step, exc=ValueError)
            check(self, who, "out.grad_log_std", g_ls, dtypes=dt, shape=(L,), rule=contiguous, exc=ValueError)
            check(self, who, "out.grad_latent", g_lat, dtypes=dt, shape=(B, L), rule=wide_rows, optional=True, exc=ValueError)
        if workspace is not None:
            need = self.sde_policy_loss_workspace_bytes(B, L)
            check(self, who, f"workspace (sde_policy_loss_workspace({B}, {L}))", workspace, dtypes=(torch.uint8,), rule=contiguous, exc=ValueError)
            if workspace.numel() < need:
                raise ValueError(f"{who}: workspace has {workspace.numel()} bytes, a batch of {B} at latent width {L} needs {need}")
        else:
            workspace = self.sde_policy_loss_workspace(B, L)
        if out is None:
            with torch.cuda.device(self.device):
                stats = torch.empty(8, dtype=torch.float64, device=self.device)
                g_in = torch.empty(B, dtype=x.dtype, device=self.device)
                g_val = torch.empty(B, dtype=x.dtype, device=self.device)
                g_ls = torch.empty(L, dtype=x.dtype, device=self.device)
                g_lat = torch.empty((B, L), dtype=x.dtype, device=self.device) if want_grad_latent else None
        d = _lib.PtgSdeLoss(kind=_lib.LOSS_PPO if ppo else _lib.LOSS_A2C,
                            flags=(_lib.LOSS_NORM_ADV if normalize_advantage else 0) | (_lib.LOSS_CLIP_VF if clip_range_vf is not None else 0),
                            in_dtype=_out_code(torch, x.dtype), latent_dim=L, batch=B, mean_dev=_ptr(x), mean_s_n=max(x.stride(0), 1),
                            val_dev=_ptr(values), val_s_n=max(values.stride(0), 1), latent_dev=_ptr(latent), latent_s_n=_row_stride(latent),
                            log_std_dev=_ptr(log_std), act_dev=_ptr(actions), old_logp_dev=_ptr(old_log_prob if ppo else None), adv_dev=_ptr(advantages),
                            ret_dev=_ptr(returns), old_val_dev=_ptr(old_values if clip_range_vf is not None else None),
                            clip_range=float(clip_range) if ppo else 0.0, clip_range_vf=float(clip_range_vf) if clip_range_vf is not None else 0.0,
                            ent_coef=float(ent_coef), vf_coef=float(vf_coef), stats_dev=_ptr(stats), grad_in_dev=_ptr(g_in), g_s_n=max(g_in.stride(0), 1),
                            grad_val_dev=_ptr(g_val), gv_s_n=max(g_val.stride(0), 1), grad_log_std_dev=_ptr(g_ls), grad_latent_dev=_ptr(g_lat),
                            gl_s_n=0 if g_lat is None else _row_stride(g_lat), ws_dev=_ptr(workspace))
        self._call("ptg_sde_policy_loss", C.byref(d))
        return SdePolicyLoss(stats, g_in, g_val, g_ls, g_lat)

    # ------------------------------------------------------------------ gSDE for SAC / TQC: the training matrix, the squashed head, its backward
    def sde_resample_rows(self, log_std, counter, noise, seed=0):
        """sde_resample for a matrix of batch rows (include/ptg_env.h: ptg_sde_resample_rows): noise [rows, L] or one row [L] is filled
        with exp(log_std[k]) * z, z the draw of (seed, *counter, r * 1024 + k) -- no global env offset, rows not tied to n_envs.  SAC /
        TQC with gSDE draw ONE row per gradient step.  The counter advances by one on the device.  Returns noise."""
        torch = self._torch
        who = "sde_resample_rows"
        log_std, L = self._sde_log_std(who, log_std, (torch.float32, torch.float64))
        check(self, who, "counter (new_draw_counter())", counter, dtypes=(torch.int64,), numel=1, shape=(1,))
        m = noise[None, :] if _dims(self, noise) == 1 else noise
        check(self, who, "noise", m, dtypes=(log_std.dtype,), shape=(None, L), rule=wide_rows, exc=ValueError)
        if m.shape[0] < 1:
            raise ValueError(f"{who}: noise has no rows, shape {tuple(noise.shape)}")
        d = _lib.PtgSdeNoise(in_dtype=_out_code(torch, log_std.dtype), latent_dim=L, log_std_dev=_ptr(log_std), seed=int(seed) & (2 ** 64 - 1),
                             counter_dev=_ptr(counter), e_dev=_ptr(m), e_s_n=_row_stride(m))
        self._call("ptg_sde_resample_rows", C.byref(d), m.shape[0])
        return noise

    def _sde_rs_inputs(self, who, mean, latent, log_std, noise, clip_mean, deterministic):
        """the checked inputs the forward and the backward share -> (mean [B], B, L, log_std [L], the flags, clip_mean)"""
        torch = self._torch
        m = check(self, who, "mean", _column(self, mean), dtypes=(torch.float32, torch.float64), shape=(None,), rule=step)
        B = m.shape[0]
        if B < 1:
            raise ValueError(f"{who}: an empty batch, mean has shape {tuple(mean.shape)}")
        dt = (m.dtype,)
        log_std, L = self._sde_log_std(who, log_std, dt)
        check(self, who, "latent", latent, dtypes=dt, shape=(B, L), rule=wide_rows)
        flags = _lib.SDE_RS_DETERMINISTIC if deterministic else 0
        if not deterministic:
            if noise is None:
                raise ValueError(f"{who}: a stochastic call needs the exploration matrix (sde_resample / sde_resample_rows)")
            if _dims(self, noise) == 1:
                check(self, who, "noise (one shared row)", noise, dtypes=dt, shape=(L,), rule=contiguous)
                flags |= _lib.SDE_RS_SHARED_E
            else:
                check(self, who, "noise", noise, dtypes=dt, shape=(B, L), rule=wide_rows)
        c = float(clip_mean)
        if not c > 0.0:
            raise ValueError(f"{who}: clip_mean must be > 0 (float('inf'): no clipping), got {clip_mean}")
        return m, B, L, log_std, flags, c

    def sde_rsample(self, mean, latent, log_std, noise, clip_mean=2.0, deterministic=False, out=None, want_step_actions=False, want_logp=True,
                    want_saved=True):
        """gSDE's squashed head as SAC / TQC use it, in one launch (include/ptg_env.h: ptg_sde_rsample): a = tanh(hardtanh(mean,
        +-clip_mean) + latent . E) and log pi(a) with SB3's tanh correction, the variance (latent^2) . exp(log_std)^2 + 1e-6.  mean [B]
        / [B, 1] (any stride >= 1): the UNCLIPPED output of the mu layer; latent [B, L] (unit column stride, row stride >= L); log_std
        [L] / [L, 1], not clamped; noise: ONE row [L] shared by the batch (training: sde_resample_rows) or a matrix [B, L] (collecting:
        sde_resample), None when deterministic; all of ONE dtype, float32 or float64.  B is not tied to n_envs.  Returns
        SdeRSample(actions, step_actions float32 or None, log_prob or None, saved float64 [B, 2] or None: what sde_rsample_backward
        reads).  out: an earlier result, reused by a captured call (its None fields are not written).  No synchronisation; a non-finite
        row or a NaN / +Inf log_std gives NaN outputs and PTG_E_NONFINITE at the next sync()."""
        torch = self._torch
        who = "sde_rsample"
        m, B, L, log_std, flags, c = self._sde_rs_inputs(who, mean, latent, log_std, noise, clip_mean, deterministic)
        specs = [("actions", True, m.dtype), ("step_actions", want_step_actions, torch.float32), ("log_prob", want_logp, m.dtype)]
        if out is not None:
            act, sact, lp, saved = _out_tuple(self, who, out, SdeRSample, stats=False)
            if act is None:
                raise ValueError(f"{who}: out.actions is missing")
            for (name, _, dt), x in zip(specs, (act, sact, lp)):
                check(self, who, f"out.{name}", _column(self, x), dtypes=(dt,), shape=(B,), rule=contiguous, optional=True, exc=ValueError)
            check(self, who, "out.saved", saved, dtypes=(torch.float64,), shape=(B, 2), rule=contiguous, optional=True, exc=ValueError)
        else:
            with torch.cuda.device(self.device):
                act, sact, lp = (torch.empty(B, dtype=dt, device=self.device) if wanted else None for _, wanted, dt in specs)
                saved = torch.empty((B, 2), dtype=torch.float64, device=self.device) if want_saved else None
        stochastic = not deterministic
        shared = bool(flags & _lib.SDE_RS_SHARED_E)
        d = _lib.PtgSdeRs(flags=flags, in_dtype=_out_code(torch, m.dtype), latent_dim=L, batch=B, mean_dev=_ptr(m), mean_s_n=max(m.stride(0), 1),
                          latent_dev=_ptr(latent), latent_s_n=_row_stride(latent), e_dev=_ptr(noise if stochastic else None),
                          e_s_n=_row_stride(noise) if stochastic and not shared else 0, log_std_dev=_ptr(log_std), clip_mean=c, act_dev=_ptr(act),
                          step_act_dev=_ptr(sact), logp_dev=_ptr(lp), saved_dev=_ptr(saved))
        self._call("ptg_sde_rsample", C.byref(d))
        return SdeRSample(act, sact, lp, saved)

    @staticmethod
    def sde_rsample_backward_workspace_bytes(batch, latent_dim):
        """ptg_sde_rsample_backward_workspace restated: 8 * L * (1 + n) with n blocks of 4 * ceil(B / 4096) rows; -1 outside the ranges
        the library accepts"""
        B, L = int(batch), int(latent_dim)
        if not (1 <= B <= 2 ** 31 and 1 <= L <= _lib.MLP_MAX_WIDTH):
            return -1
        per = 4 * ((B - 1) // 4096 + 1)
        return 8 * L * (1 + (B - 1) // per + 1)

    def sde_rsample_backward_workspace(self, batch, latent_dim):
        """the device scratch of sde_rsample_backward for a batch of this size and latent width (a uint8 tensor)"""
        nbytes = self._L.ptg_sde_rsample_backward_workspace(int(batch), int(latent_dim))
        if nbytes < 0:
            raise ValueError(f"sde_rsample_backward_workspace: batch must be in [1, 2^31] and latent_dim in [1, {_lib.MLP_MAX_WIDTH}], got {batch}, {latent_dim}")
        with self._torch.cuda.device(self.device):
            return self._torch.empty(nbytes, dtype=self._torch.uint8, device=self.device)

    def sde_rsample_backward(self, mean, latent, log_std, noise, saved, grad_actions, grad_log_prob, clip_mean=2.0, deterministic=False,
                             want_grad_latent=True, want_grad_log_std=True, out=None, workspace=None):
        """The backward of sde_rsample (include/ptg_env.h: ptg_sde_rsample_backward): from the same mean, latent, log_std and noise, the
        (noise, V) pairs the forward saved and the incoming gradients d L / d actions and d L / d log_prob ([B] or [B, 1], contiguous;
        either may be None = 0, not both), the gradients with respect to the unclipped mean (0 outside the open interval
        +-clip_mean), the latent [B, L] (through the variance and through the noise) and log_std [L] (through the variance and through
        the matrix row E = exp(log_std) * z itself; only with one shared row).  Returns SdeRSampleGrad(grad_mean [B], grad_latent or
        None, grad_log_std or None); out: such a tuple; workspace: sde_rsample_backward_workspace(B, L) or larger.  No synchronisation;
        a bad row gives NaN gradients, a NaN grad_log_std and PTG_E_NONFINITE at the next sync()."""
        torch = self._torch
        who = "sde_rsample_backward"
        m, B, L, log_std, flags, c = self._sde_rs_inputs(who, mean, latent, log_std, noise, clip_mean, deterministic)
        dt = (m.dtype,)
        shared = bool(flags & _lib.SDE_RS_SHARED_E)
        check(self, who, "saved", saved, dtypes=(torch.float64,), shape=(B, 2), rule=contiguous)
        ga = check(self, who, "grad_actions", _column(self, grad_actions), dtypes=dt, shape=(B,), rule=contiguous, optional=True)
        gl = check(self, who, "grad_log_prob", _column(self, grad_log_prob), dtypes=dt, shape=(B,), rule=contiguous, optional=True)
        if ga is None and gl is None:
            raise ValueError(f"{who}: grad_actions and grad_log_prob are both None")
        if out is not None:
            gm, g_lat, g_ls = _out_tuple(self, who, out, SdeRSampleGrad, stats=False)
            gm = check(self, who, "out.grad_mean", _column(self, gm), dtypes=dt, shape=(B,), rule=step, exc=ValueError)
            check(self, who, "out.grad_latent", g_lat, dtypes=dt, shape=(B, L), rule=wide_rows, optional=True, exc=ValueError)
            check(self, who, "out.grad_log_std", g_ls, dtypes=dt, shape=(L,), rule=contiguous, optional=True, exc=ValueError)
            want_grad_log_std = g_ls is not None
        if want_grad_log_std and not shared:
            raise ValueError(f"{who}: the log_std gradient needs one shared noise row [L]; a collecting matrix (or no noise) has no such backward")
        need = self.sde_rsample_backward_workspace_bytes(B, L)
        if workspace is not None:
            check(self, who, f"workspace (sde_rsample_backward_workspace({B}, {L}))", workspace, dtypes=(torch.uint8,), rule=contiguous, exc=ValueError)
            if workspace.numel() < need:
                raise ValueError(f"{who}: workspace has {workspace.numel()} bytes, a batch of {B} at latent width {L} needs {need}")
        else:
            workspace = self.sde_rsample_backward_workspace(B, L)
        if out is None:
            with torch.cuda.device(self.device):
                gm = torch.empty(B, dtype=m.dtype, device=self.device)
                g_lat = torch.empty((B, L), dtype=m.dtype, device=self.device) if want_grad_latent else None
                g_ls = torch.empty(L, dtype=m.dtype, device=self.device) if want_grad_log_std else None
        stochastic = not deterministic
        d = _lib.PtgSdeRs(flags=flags, in_dtype=_out_code(torch, m.dtype), latent_dim=L, batch=B, mean_dev=_ptr(m), mean_s_n=max(m.stride(0), 1),
                          latent_dev=_ptr(latent), latent_s_n=_row_stride(latent), e_dev=_ptr(noise if stochastic else None),
                          e_s_n=_row_stride(noise) if stochastic and not shared else 0, log_std_dev=_ptr(log_std), clip_mean=c, saved_dev=_ptr(saved),
                          grad_act_dev=_ptr(ga), grad_logp_dev=_ptr(gl), grad_mean_dev=_ptr(gm), gm_s_n=max(gm.stride(0), 1),
                          grad_latent_dev=_ptr(g_lat), gl_s_n=0 if g_lat is None else _row_stride(g_lat), grad_log_std_dev=_ptr(g_ls), ws_dev=_ptr(workspace))
        self._call("ptg_sde_rsample_backward", C.byref(d))
        return SdeRSampleGrad(gm, g_lat, g_ls)

    # ------------------------------------------------------------------ the TD loss of a replay batch and its gradients
    def td_loss_workspace(self, batch):
        """the device scratch of td_loss for a batch of this size (a uint8 tensor; reuse it across calls of up to that size)"""
        return self._loss_workspace("td_loss", batch)

    def td_loss(self, kind, q, next_q, rewards, dones, gamma, *, actions=None, next_log_prob=None, ent_coef=None, log_ent_coef=None,
                want_target=False, out=None, workspace=None):
        """Enqueue, on the current stream, the TD target and the loss lines of SB3's DQN.train (kind "dqn"), TD3.train ("td3") or
        SAC.train ("sac") on one replay batch together with their gradients with respect to the current Q-values (include/ptg_env.h:
        ptg_td_loss, which states the arithmetic).
        "dqn": q = Q(s, .) and next_q = Q_target(s', .), both [B, A] (2 <= A <= 32, unit column stride, row stride >= A) of one float
        dtype, with int32 / int64 actions [B].  "td3" / "sac": q and next_q are lists of K tensors (1 <= K <= 4), [B] or [B, 1] each
        with any stride >= 1 -- SB3's tuples of critic outputs, or the columns of one [B, K] tensor; "sac" also takes next_log_prob [B]
        in the Q dtype and exactly one of ent_coef (a Python float, kept by a captured call, or a float64 device tensor of 1 element,
        read when the kernel runs) and log_ent_coef (a float64 device tensor of 1 element holding log alpha: SAC's learned
        parameter).  rewards and dones: contiguous [B] (or [B, 1]), float32 or float64 each on its own -- what
        DeviceReplayBuffer.sample() returns.  gamma: a finite Python float.
        Returns TdLoss(stats float64 [8] = loss, mean current Q, mean target, mean |delta|, share of |delta| >= 1, alpha as used, 0, 0;
        grad_q = d loss / d q, a tensor for "dqn" and a list for the critics; target [B] with want_target, else None).  out: an earlier
        result, reused by a captured call (its target, when not None, is written); workspace: td_loss_workspace(B) or larger,
        allocated when missing.  Fresh gradients are torch.empty: a row refused for its action keeps what was there.  Outputs must
        not overlap each other or the inputs: a tensor given twice is refused, any other overlap is not checked.  No
        synchronisation; a bad row makes the next sync() raise PtgError (PTG_E_INDEX / PTG_E_NONFINITE)."""
        d, res, _ = self._td_loss_member("td_loss", kind, q, next_q, rewards, dones, gamma, actions=actions, next_log_prob=next_log_prob, ent_coef=ent_coef,
                                         log_ent_coef=log_ent_coef, want_target=want_target, out=out, workspace=workspace)[1]()
        self._call("ptg_td_loss", C.byref(d))
        return res

    def _td_loss_member(self, who, kind, q, next_q, rewards, dones, gamma, *, actions=None, next_log_prob=None, ent_coef=None, log_ent_coef=None,
                        want_target=False, out=None, workspace=None):
        """Every check of ONE TD-loss call, in td_loss's order, for td_loss and for each member of td_loss_group (who: "td_loss", or
        "td_loss_group: member i").  Allocates nothing and does not touch the library.  Returns (what a group must agree in, as (name,
        value) pairs; make; the outputs and workspace the caller gave), where make() allocates what was not given and returns (the
        PtgTd, the TdLoss, the workspace, which must outlive the library call)."""
        torch = self._torch
        if kind not in ("dqn", "td3", "sac"):
            raise ValueError(f"{who}: kind must be 'dqn', 'td3' or 'sac', got {kind!r}")
        dqn, sac = kind == "dqn", kind == "sac"
        floats = (torch.float32, torch.float64)
        if dqn:
            x = check(self, who, "q", q, dtypes=floats, shape=(None, None), rule=rows)
            B, A = x.shape
            if not 2 <= A <= 32:
                raise ValueError(f"{who}: q must be [B, A] with 2 <= A <= 32, got shape {tuple(x.shape)}")
            dt = (x.dtype,)
            qs, nqs = [x], [check(self, who, "next_q", next_q, dtypes=dt, shape=(B, A), rule=rows)]
        else:
            for name, xs in (("q", q), ("next_q", next_q)):
                if not isinstance(xs, (list, tuple)):
                    raise TypeError(f"{who}: {name} must be a list of critic outputs for kind {kind!r}, got {type(xs).__name__}")
            if not 1 <= len(q) <= _lib.TD_MAX_CRITICS or len(next_q) != len(q):
                raise ValueError(f"{who}: q and next_q must hold the same number of critics, 1 to {_lib.TD_MAX_CRITICS}, got {len(q)} and {len(next_q)}")
            A = 0
            qs = _critic_columns(self, who, "q", q, floats)
            x = qs[0]
            (B,), dt = x.shape, (x.dtype,)
            nqs = _critic_columns(self, who, "next_q", next_q, dt, B)
        if B < 1:
            raise ValueError(f"{who}: an empty batch, q has shape {tuple(x.shape)}")
        K = len(qs)
        rewards = check(self, who, "rewards", _column(self, rewards), dtypes=floats, shape=(B,), rule=contiguous)
        dones = check(self, who, "dones", _column(self, dones), dtypes=floats, shape=(B,), rule=contiguous)
        if dqn != (actions is not None):
            raise ValueError(f"{who}: actions go with kind 'dqn' and with no other")
        if sac != (next_log_prob is not None):
            raise ValueError(f"{who}: next_log_prob goes with kind 'sac' and with no other")
        if (ent_coef is not None) + (log_ent_coef is not None) != (1 if sac else 0):
            raise ValueError(f"{who}: kind 'sac' takes exactly one of ent_coef and log_ent_coef, the other kinds neither")
        if not np.isfinite(float(gamma)):
            raise ValueError(f"{who}: gamma must be finite, got {gamma}")
        actions = check(self, who, "actions", _column(self, actions), dtypes=(torch.int32, torch.int64), shape=(B,), rule=contiguous, optional=True)
        next_log_prob = check(self, who, "next_log_prob", _column(self, next_log_prob), dtypes=dt, shape=(B,), rule=contiguous, optional=True)
        alpha_dev, alpha = _alpha_arg(self, who, ent_coef, log_ent_coef)
        if out is not None:
            stats, g_q, target = _out_tuple(self, who, out, TdLoss)
            if dqn:
                gs = [check(self, who, "out.grad_q", g_q, dtypes=dt, shape=(B, A), rule=rows, exc=ValueError)]
            else:
                if not isinstance(g_q, (list, tuple)) or len(g_q) != K:
                    raise ValueError(f"{who}: out.grad_q must be a list of {K} tensors")
                gs = _critic_columns(self, who, "out.grad_q", g_q, dt, B, exc=ValueError)
            if want_target and target is None:
                raise ValueError(f"{who}: want_target, but out.target is None")
            check(self, who, "out.target", target, dtypes=dt, shape=(B,), rule=contiguous, optional=True, exc=ValueError)
            _no_tensor_twice(who, gs + qs + nqs + ([target] if target is not None else []), "out.grad_q, out.target, q and next_q")
        self._take_workspace("td_loss", B, workspace, who=who, fresh=False)
        agree = (("kind", kind), ("the number of actions", A), ("the number of critics", K), ("the dtype", x.dtype), ("the rewards' dtype", rewards.dtype),
                 ("the dones' dtype", dones.dtype), ("the actions' dtype", actions.dtype if dqn else None), ("log_ent_coef given or not", log_ent_coef is not None),
                 ("the batch", B))
        theirs = None if out is None else (stats, g_q, gs, target)
        given = ([] if out is None else [stats] + list(gs) + ([target] if target is not None else [])) + ([] if workspace is None else [workspace])

        def make():
            ws = self._loss_workspace("td_loss", B) if workspace is None else workspace
            if theirs is None:
                with torch.cuda.device(self.device):
                    stats = torch.empty(8, dtype=torch.float64, device=self.device)
                    g_q = [torch.empty(tuple(t.shape), dtype=x.dtype, device=self.device) for t in ([q] if dqn else q)]
                    gs = g_q if dqn else [_column(self, t) for t in g_q]
                    g_q = g_q[0] if dqn else g_q
                    target = torch.empty(B, dtype=x.dtype, device=self.device) if want_target else None
            else:
                stats, g_q, gs, target = theirs
            d = _lib.PtgTd(kind=_lib.TD_DQN if dqn else _lib.TD_CRITICS,
                           flags=(_lib.TD_ENTROPY if sac else 0) | (_lib.TD_LOG_ALPHA if log_ent_coef is not None else 0),
                           n_actions=A, n_critics=0 if dqn else K, q_dtype=_out_code(torch, x.dtype),
                           act_kind=_lib.ACT_I64 if dqn and actions.dtype == torch.int64 else _lib.ACT_I32,
                           rew_dtype=_out_code(torch, rewards.dtype), done_dtype=_out_code(torch, dones.dtype), batch=B,
                           act_dev=_ptr(actions), rew_dev=_ptr(rewards), done_dev=_ptr(dones), next_logp_dev=_ptr(next_log_prob),
                           alpha_dev=_ptr(alpha_dev), gamma=float(gamma), alpha=alpha, scale=0.5 if sac else 1.0,
                           stats_dev=_ptr(stats), y_dev=_ptr(target), ws_dev=_ptr(ws))
            least = max(A, 1)
            for k in range(K):
                d.q_dev[k], d.q_s_n[k] = qs[k].data_ptr(), max(qs[k].stride(0), least)
                d.next_q_dev[k], d.next_s_n[k] = nqs[k].data_ptr(), max(nqs[k].stride(0), least)
                d.grad_q_dev[k], d.g_s_n[k] = gs[k].data_ptr(), max(gs[k].stride(0), least)
            return d, TdLoss(stats, g_q, target), ws
        return agree, make, given

    def td_loss_group(self, kind, members, *, gamma=None, ent_coef=None, want_target=False):
        """td_loss for G independent replay batches of ONE batch size, 1 <= G <= 8, in exactly the launches of one td_loss call
        (include/ptg_env.h: ptg_td_loss_group): the agents of a seed sweep.  Every member's result is, bit for bit,
        what td_loss gives for its arguments.  members: a list of G dicts of td_loss's arguments by name (q, next_q, rewards, dones, and
        any of gamma, actions, next_log_prob, ent_coef, log_ent_coef, want_target, out, workspace); gamma, ent_coef and want_target here
        are one value for the members that do not name them, or a list with one entry per member.  The members must agree in kind, A, K,
        the dtypes, whether log_ent_coef is given, and B (ValueError, which names the two members); every scalar may differ, and one
        member may bring a float ent_coef where another brings a device tensor.  No tensor may serve two members as an output or
        workspace.  Checked as td_loss checks, member by member, the message behind "member i:"; the library is not touched and nothing is
        allocated before every check has passed, and nothing at all when every member brings out= and workspace=.  Returns the list of G
        TdLoss.  Cost: profiles/offpolicy_group_cost.txt; DESIGN.md section 27."""
        made = self._train_group("td_loss_group", "td_loss", members, ("q", "next_q", "rewards", "dones", "gamma"),
                                 ("actions", "next_log_prob", "ent_coef", "log_ent_coef", "want_target", "out", "workspace"),
                                 dict(gamma=gamma, ent_coef=ent_coef, want_target=want_target), lambda who, kw: self._td_loss_member(who, kind, **kw))
        self._call("ptg_td_loss_group", (_lib.PtgTd * len(made))(*[m[0] for m in made]), len(made))      # made holds the workspaces until here
        return [m[1] for m in made]

    def _train_group(self, who, single, members, needs, takes, shared, member):
        """What the grouped off-policy ops share: the members' container and count, the keyword defaults (one value, or a list with one
        per member; None: no default), every member through the single op's check function member(who_i, kwargs) in order, the
        agreement, no output or workspace twice -- then, and only then, every member's make().  Returns the list of what make() gave."""
        if not isinstance(members, (list, tuple)) or not all(isinstance(m, dict) for m in members):
            raise TypeError(f"{who}: members must be a list of dicts of {single}'s arguments, got {type(members).__name__}")
        G = len(members)
        if not 1 <= G <= _lib.TRAIN_GROUP_MAX:
            raise ValueError(f"{who}: 1 to {_lib.TRAIN_GROUP_MAX} members, got {G}")
        for name, v in shared.items():
            if isinstance(v, list) and len(v) != G:
                raise ValueError(f"{who}: {name} must have one entry per member, {G}, or be one value for all; got {len(v)}")
        checked = []
        for i, m in enumerate(members):
            kw = {name: (v[i] if isinstance(v, list) else v) for name, v in shared.items() if v is not None}
            kw.update(m)
            missing, unknown = [k for k in needs if k not in kw], [k for k in kw if k not in needs and k not in takes]
            if missing or unknown:
                raise TypeError(f"{who}: member {i}: a member names {single}'s arguments; missing {missing}, unknown {unknown}")
            checked.append(member(f"{who}: member {i}", kw))
        for i, (agree, _, _) in enumerate(checked):
            for (name, a), (_, b) in zip(checked[0][0], agree):
                if a != b:
                    raise ValueError(f"{who}: members 0 and {i} disagree in {name}: {a} and {b}")
        _no_tensor_twice(who, [t for _, _, given in checked for t in given], "the members' outputs, counters and workspaces")
        return [make() for _, make, _ in checked]

    # ------------------------------------------------------------------ TQC's quantile-Huber critic loss and its gradients
    def quantile_loss_workspace(self, batch):
        """the device scratch of quantile_loss for a batch of this size (a uint8 tensor; reuse it across calls of up to that size)"""
        return self._loss_workspace("quantile_loss", batch)

    def _quantile_views(self, who, name, x, dtypes, B=None, K=None, Q=None, exc=TypeError):
        """a [B, K, Q] tensor or a list of K [B, Q] tensors -> the K checked [B, Q] views"""
        if isinstance(x, (list, tuple)):
            if not 1 <= len(x) <= _lib.TD_MAX_CRITICS or (K is not None and len(x) != K):
                raise ValueError(f"{who}: {name} must hold {K if K is not None else f'1 to {_lib.TD_MAX_CRITICS}'} critics, got {len(x)}")
            views = []
            for k, t in enumerate(x):
                views.append(check(self, who, f"{name}[{k}]", t, dtypes=dtypes, shape=(B, Q), rule=rows, exc=exc))
                if k == 0:
                    dtypes, (B, Q) = (t.dtype,), t.shape
            return views
        x = check(self, who, name, x, dtypes=dtypes, shape=(B, K, Q), rule=stacked, exc=exc)
        if not 1 <= x.shape[1] <= _lib.TD_MAX_CRITICS:
            raise ValueError(f"{who}: {name} must be [B, K, Q] with 1 <= K <= {_lib.TD_MAX_CRITICS}, got shape {tuple(x.shape)}")
        return [x[:, k] for k in range(x.shape[1])]

    def quantile_loss(self, quantiles, next_quantiles, rewards, dones, next_log_prob, gamma, top_quantiles_to_drop_per_net, *, ent_coef=None,
                      log_ent_coef=None, out=None, workspace=None, want_target=False):
        """Enqueue, on the current stream, the critic lines of sb3_contrib's TQC.train on one replay batch -- the sort of the target
        critics' quantiles, the drop of the top ones, the entropy term, the TD targets and quantile_huber_loss(sum_over_quantiles=False)
        -- together with the gradients with respect to the current quantiles (include/ptg_env.h: ptg_quantile_loss, which states the
        arithmetic).
        quantiles (current critics on (s, a)) and next_quantiles (target critics on (s', a')): a [B, K, Q] tensor with unit stride along
        Q and a row stride >= Q, or a list of K [B, Q] tensors with unit column stride and a row stride >= Q each; 1 <= K <= 4,
        1 <= Q <= 64, one float dtype for both.  top_quantiles_to_drop_per_net: an int d, 0 <= d < Q; M = K * (Q - d) targets are kept.
        rewards and dones: contiguous [B] (or [B, 1]), float32 or float64 each on its own -- what DeviceReplayBuffer.sample() returns;
        next_log_prob [B] (or [B, 1]) in the quantiles' dtype.  Exactly one of ent_coef (a Python float, kept by a captured call, or a
        float64 device tensor of 1 element, read when the kernel runs) and log_ent_coef (a float64 device tensor of 1 element holding
        log alpha).  gamma: a finite Python float.
        Returns QuantileLoss(stats float64 [8] = loss, mean current quantile, mean target, mean |delta|, share of the pairs with
        |delta| > 1, alpha as used, 0, 0; grad_quantiles = d loss / d quantiles, a tensor or a list as the quantiles came; target
        [B, M] with want_target, else None).  out: an earlier result, reused by a captured call (its target, when not None, is
        written); workspace: quantile_loss_workspace(B) or larger, allocated when missing.  Outputs must not overlap each other or the
        inputs: a tensor given twice is refused, any other overlap is not checked.  No synchronisation; a non-finite row makes the
        next sync() raise PtgError (PTG_E_NONFINITE)."""
        torch = self._torch
        who = "quantile_loss"
        floats = (torch.float32, torch.float64)
        as_list = isinstance(quantiles, (list, tuple))
        cur = self._quantile_views(who, "quantiles", quantiles, floats)
        (B, Q), K, dt = cur[0].shape, len(cur), (cur[0].dtype,)
        if B < 1 or not 1 <= Q <= _lib.QL_MAX_QUANTILES:
            raise ValueError(f"{who}: quantiles need B >= 1 and 1 <= Q <= {_lib.QL_MAX_QUANTILES}, got B = {B}, Q = {Q}")
        nxt = self._quantile_views(who, "next_quantiles", next_quantiles, dt, B, K, Q)
        rewards = check(self, who, "rewards", _column(self, rewards), dtypes=floats, shape=(B,), rule=contiguous)
        dones = check(self, who, "dones", _column(self, dones), dtypes=floats, shape=(B,), rule=contiguous)
        next_log_prob = check(self, who, "next_log_prob", _column(self, next_log_prob), dtypes=dt, shape=(B,), rule=contiguous)
        drop = top_quantiles_to_drop_per_net
        if isinstance(drop, bool) or not isinstance(drop, (int, np.integer)):
            raise TypeError(f"{who}: top_quantiles_to_drop_per_net must be an int, got {type(drop).__name__}")
        if not 0 <= drop < Q:
            raise ValueError(f"{who}: top_quantiles_to_drop_per_net must be in [0, {Q}), got {drop}")
        M = K * (Q - int(drop))
        if (ent_coef is not None) + (log_ent_coef is not None) != 1:
            raise ValueError(f"{who}: exactly one of ent_coef and log_ent_coef")
        if not np.isfinite(float(gamma)):
            raise ValueError(f"{who}: gamma must be finite, got {gamma}")
        alpha_dev, alpha = _alpha_arg(self, who, ent_coef, log_ent_coef)
        if out is not None:
            stats, g_q, target = _out_tuple(self, who, out, QuantileLoss)
            if isinstance(g_q, (list, tuple)) != as_list:
                raise ValueError(f"{who}: out.grad_quantiles must be a {'list of ' + str(K) + ' tensors' if as_list else 'tensor'}, as the quantiles are")
            gs = self._quantile_views(who, "out.grad_quantiles", g_q, dt, B, K, Q, exc=ValueError)
            if want_target and target is None:
                raise ValueError(f"{who}: want_target, but out.target is None")
            check(self, who, "out.target", target, dtypes=dt, shape=(B, M), rule=contiguous, optional=True, exc=ValueError)
            _no_tensor_twice(who, gs + cur + nxt + ([target] if target is not None else []), "out.grad_quantiles, out.target, quantiles and next_quantiles")
        workspace = self._take_workspace(who, B, workspace)
        if out is None:
            with torch.cuda.device(self.device):
                stats = torch.empty(8, dtype=torch.float64, device=self.device)
                g_q, gs = self._fresh_like_quantiles(as_list, B, K, Q, dt[0])
                target = torch.empty((B, M), dtype=dt[0], device=self.device) if want_target else None
        d = _lib.PtgQl(flags=_lib.QL_LOG_ALPHA if log_ent_coef is not None else 0, n_critics=K, n_quantiles=Q, n_drop=int(drop),
                       q_dtype=_out_code(torch, dt[0]), rew_dtype=_out_code(torch, rewards.dtype), done_dtype=_out_code(torch, dones.dtype), batch=B,
                       rew_dev=_ptr(rewards), done_dev=_ptr(dones), next_logp_dev=_ptr(next_log_prob), alpha_dev=_ptr(alpha_dev), gamma=float(gamma),
                       alpha=alpha, stats_dev=_ptr(stats), y_dev=_ptr(target), ws_dev=_ptr(workspace))
        for k in range(K):
            d.cur_dev[k], d.cur_s_n[k] = cur[k].data_ptr(), max(cur[k].stride(0), Q)
            d.next_dev[k], d.next_s_n[k] = nxt[k].data_ptr(), max(nxt[k].stride(0), Q)
            d.grad_dev[k], d.g_s_n[k] = gs[k].data_ptr(), max(gs[k].stride(0), Q)
        self._call("ptg_quantile_loss", C.byref(d))
        return QuantileLoss(stats, g_q, target)

    # ------------------------------------------------------------------ the training-time actor head: SAC / TQC rsample, TD3's target action
    def _rs_rows(self, who, mean, log_std):
        """mean and log_std [B] / [B, 1] of one float dtype, any stride >= 1 -> their [B] views and B"""
        torch = self._torch
        m = check(self, who, "mean", _column(self, mean), dtypes=(torch.float32, torch.float64), shape=(None,), rule=step)
        B = m.shape[0]
        ls = check(self, who, "log_std", _column(self, log_std), dtypes=(m.dtype,), shape=(B,), rule=step) if log_std is not None else None
        if B < 1:
            raise ValueError(f"{who}: an empty batch, mean has shape {tuple(mean.shape)}")
        return m, ls, B

    def rsample(self, mean, log_std, counter, seed=0, deterministic=False, out=None):
        """Enqueue, on the current stream, SB3's Actor.action_log_prob of SAC / TQC on a replay batch (include/ptg_env.h: ptg_rsample,
        which states the arithmetic): log_std clamped to [-20, 2], a = tanh(mean + exp(log_std) * z) with z the c-th Box-Muller draw of
        row b under (seed, c, b), c = the counter's value on the device (deterministic: z = 0), and log pi(a) with SB3's tanh correction.
        mean, log_std: [B] or [B, 1] of one float dtype (float32 / float64), any stride >= 1 -- B is not tied to n_envs; log_std is the
        network's unclamped output.  counter: new_draw_counter(); a stochastic call advances it by one on the device.
        Returns RSample(actions, log_prob in the inputs' dtype and shaped like mean, noise float64: z, which rsample_backward reads).
        out: an earlier result, reused by a captured call; its log_prob and noise may be None (not written).  No synchronisation; a
        non-finite mean or a NaN log_std gives NaN outputs and PTG_E_NONFINITE at the next sync()."""
        d, res = self._rsample_member("rsample", mean, log_std, counter, seed=seed, deterministic=deterministic, out=out)[1]()
        self._call("ptg_rsample", C.byref(d))
        return res

    def _rsample_member(self, who, mean, log_std, counter, seed=0, deterministic=False, out=None):
        """Every check of ONE rsample call, in rsample's order, for rsample and for each member of rsample_group.  Allocates nothing and does
        not touch the library.  Returns (what a group must agree in; make; the outputs the caller gave and the counter a stochastic call
        advances), where make() allocates what was not given and returns (the PtgRs, the RSample)."""
        torch = self._torch
        m, ls, B = self._rs_rows(who, mean, log_std)
        if ls is None:
            raise TypeError(f"{who}: log_std must be a tensor, got NoneType")
        counter = self._act_counter(who, counter, deterministic)
        if out is not None:
            act, lp, noise = _out_tuple(self, who, out, RSample, stats=False)
            check(self, who, "out.actions", _column(self, act), dtypes=(m.dtype,), shape=(B,), rule=contiguous, exc=ValueError)
            check(self, who, "out.log_prob", _column(self, lp), dtypes=(m.dtype,), shape=(B,), rule=contiguous, optional=True, exc=ValueError)
            check(self, who, "out.noise", _column(self, noise), dtypes=(torch.float64,), shape=(B,), rule=contiguous, optional=True, exc=ValueError)
        agree = (("the dtype", m.dtype), ("deterministic", bool(deterministic)), ("the batch", B))
        given = ([] if out is None else [t for t in out if t is not None]) + ([] if deterministic or counter is None else [counter])

        def make():
            if out is None:
                with torch.cuda.device(self.device):
                    act, lp = (torch.empty(tuple(mean.shape), dtype=m.dtype, device=self.device) for _ in range(2))
                    noise = torch.empty(tuple(mean.shape), dtype=torch.float64, device=self.device)
            else:
                act, lp, noise = out
            d = _lib.PtgRs(kind=_lib.RS_SQUASH, flags=_lib.RS_DETERMINISTIC if deterministic else 0, q_dtype=_out_code(torch, m.dtype), batch=B,
                           mean_dev=_ptr(m), mean_s_n=max(m.stride(0), 1), log_std_dev=_ptr(ls), log_std_s_n=max(ls.stride(0), 1),
                           seed=int(seed) & (2 ** 64 - 1), counter_dev=_ptr(counter), act_dev=_ptr(act), logp_dev=_ptr(lp), noise_dev=_ptr(noise))
            return d, RSample(act, lp, noise)
        return agree, make, given

    def rsample_group(self, members, *, seed=0, deterministic=False):
        """rsample for G independent actors' outputs of ONE batch size, 1 <= G <= 8, in exactly the launches of one rsample call
        (include/ptg_env.h: ptg_rsample_group).  Every member's actions, log-probs and noise are, bit for bit, what
        rsample gives for its arguments, and every member's counter advances by one.  members: a list of G dicts of rsample's arguments
        by name (mean, log_std, counter, and any of seed, out); seed is one value for the members that do not name it, or a list with
        one per member; deterministic is the group's.  The members must agree in the dtype and B; no tensor may serve two members as an
        output, and no counter two members: the grouped call reads every counter before any is advanced.  Checked as rsample checks, member
        by member, the message behind "member i:".  Returns the list of G RSample."""
        made = self._train_group("rsample_group", "rsample", members, ("mean", "log_std", "counter"), ("seed", "out"), dict(seed=seed),
                                 lambda who, kw: self._rsample_member(who, deterministic=deterministic, **kw))
        self._call("ptg_rsample_group", (_lib.PtgRs * len(made))(*[m[0] for m in made]), len(made))
        return [m[1] for m in made]

    def rsample_backward(self, mean, log_std, noise, grad_actions, grad_log_prob, out=None):
        """Enqueue, on the current stream, the backward of rsample (include/ptg_env.h: ptg_rsample_backward): from the same mean and log_std,
        the noise rsample stored, and the incoming gradients d L / d actions and d L / d log_prob ([B] or [B, 1], contiguous, in the inputs'
        dtype; either may be None = 0, not both), the gradients with respect to mean and to the unclamped log_std (0 outside the clamp).
        Returns RSampleGrad(grad_mean, grad_log_std), shaped like mean and log_std; out: such a pair, any stride >= 1.  No synchronisation;
        a non-finite input row gives NaN gradients and PTG_E_NONFINITE at the next sync()."""
        d, res = self._rsample_backward_member("rsample_backward", mean, log_std, noise, grad_actions, grad_log_prob, out=out)[1]()
        self._call("ptg_rsample_backward", C.byref(d))
        return res

    def _rsample_backward_member(self, who, mean, log_std, noise, grad_actions, grad_log_prob, out=None):
        """Every check of ONE rsample_backward call, in its order, for rsample_backward and for each member of rsample_backward_group;
        returns (agree, make, given) as _rsample_member does, make() giving (the PtgRs, the RSampleGrad)"""
        torch = self._torch
        m, ls, B = self._rs_rows(who, mean, log_std)
        if ls is None:
            raise TypeError(f"{who}: log_std must be a tensor, got NoneType")
        dt = (m.dtype,)
        noise = check(self, who, "noise", _column(self, noise), dtypes=(torch.float64,), shape=(B,), rule=contiguous)
        ga = check(self, who, "grad_actions", _column(self, grad_actions), dtypes=dt, shape=(B,), rule=contiguous, optional=True)
        gl = check(self, who, "grad_log_prob", _column(self, grad_log_prob), dtypes=dt, shape=(B,), rule=contiguous, optional=True)
        if ga is None and gl is None:
            raise ValueError(f"{who}: grad_actions and grad_log_prob are both None")
        if out is not None:
            gm, gs = _out_tuple(self, who, out, RSampleGrad, stats=False)
            check(self, who, "out.grad_mean", _column(self, gm), dtypes=dt, shape=(B,), rule=step, exc=ValueError)
            check(self, who, "out.grad_log_std", _column(self, gs), dtypes=dt, shape=(B,), rule=step, exc=ValueError)
        agree = (("the dtype", m.dtype), ("the batch", B))
        given = [] if out is None else list(out)

        def make():
            if out is None:
                with torch.cuda.device(self.device):
                    gm = torch.empty(tuple(mean.shape), dtype=m.dtype, device=self.device)
                    gs = torch.empty(tuple(log_std.shape), dtype=m.dtype, device=self.device)
            else:
                gm, gs = out
            gm1, gs1 = _column(self, gm), _column(self, gs)
            d = _lib.PtgRs(kind=_lib.RS_SQUASH, q_dtype=_out_code(torch, m.dtype), batch=B, mean_dev=_ptr(m), mean_s_n=max(m.stride(0), 1),
                           log_std_dev=_ptr(ls), log_std_s_n=max(ls.stride(0), 1), noise_dev=_ptr(noise), grad_act_dev=_ptr(ga), grad_logp_dev=_ptr(gl),
                           grad_mean_dev=_ptr(gm1), gm_s_n=max(gm1.stride(0), 1), grad_log_std_dev=_ptr(gs1), gl_s_n=max(gs1.stride(0), 1))
            return d, RSampleGrad(gm, gs)
        return agree, make, given

    def rsample_backward_group(self, members):
        """rsample_backward for G members of ONE batch size and dtype, 1 <= G <= 8, in one launch (include/ptg_env.h:
        ptg_rsample_backward_group): every member's two gradients are, bit for bit, what rsample_backward gives for
        its arguments.  members: a list of G dicts of rsample_backward's arguments by name (mean, log_std, noise, grad_actions,
        grad_log_prob -- either may be None, member by member -- and out).  Returns the list of G RSampleGrad."""
        made = self._train_group("rsample_backward_group", "rsample_backward", members, ("mean", "log_std", "noise", "grad_actions", "grad_log_prob"), ("out",), {},
                                 lambda who, kw: self._rsample_backward_member(who, **kw))
        self._call("ptg_rsample_backward_group", (_lib.PtgRs * len(made))(*[m[0] for m in made]), len(made))
        return [m[1] for m in made]

    def smooth_target_action(self, mean, counter, noise_std, noise_clip, clip=(-1.0, 1.0), seed=0, out=None):
        """Enqueue, on the current stream, TD3.train's target-policy smoothing (include/ptg_env.h: ptg_rsample, PTG_RS_SMOOTH):
        clip(mean + clip(noise_std * z, -noise_clip, noise_clip), clip[0], clip[1]) with rsample's draw.  mean = actor_target(next_obs),
        [B] or [B, 1], float32 / float64, any stride >= 1.  Returns the actions, shaped like mean (out: such a tensor, contiguous).
        The counter advances by one on the device.  No synchronisation; a non-finite mean gives NaN and PTG_E_NONFINITE at the next sync()."""
        d, res = self._smooth_member("smooth_target_action", mean, counter, noise_std, noise_clip, clip=clip, seed=seed, out=out)[1]()
        self._call("ptg_rsample", C.byref(d))
        return res

    def _smooth_member(self, who, mean, counter, noise_std, noise_clip, clip=(-1.0, 1.0), seed=0, out=None):
        """Every check of ONE smooth_target_action call, in its order, for it and for each member of smooth_target_action_group; returns
        (agree, make, given) as _rsample_member does, make() giving (the PtgRs, the actions)"""
        torch = self._torch
        m, _, B = self._rs_rows(who, mean, None)
        counter = self._act_counter(who, counter, False)
        sd, c, lo, hi = float(noise_std), float(noise_clip), float(clip[0]), float(clip[1])
        if not (0.0 <= sd < float("inf")) or not c >= 0.0:
            raise ValueError(f"{who}: noise_std must be finite and >= 0 and noise_clip >= 0, got {noise_std} and {noise_clip}")
        if not lo <= hi:
            raise ValueError(f"{who}: clip {clip} is not an interval")
        check(self, who, "out", _column(self, out), dtypes=(m.dtype,), shape=(B,), rule=contiguous, optional=True, exc=ValueError)
        agree = (("the dtype", m.dtype), ("the batch", B))
        given = ([] if out is None else [out]) + [counter]

        def make():
            act = out
            if act is None:
                with torch.cuda.device(self.device):
                    act = torch.empty(tuple(mean.shape), dtype=m.dtype, device=self.device)
            d = _lib.PtgRs(kind=_lib.RS_SMOOTH, q_dtype=_out_code(torch, m.dtype), batch=B, mean_dev=_ptr(m), mean_s_n=max(m.stride(0), 1),
                           seed=int(seed) & (2 ** 64 - 1), counter_dev=_ptr(counter), noise_std=sd, noise_clip=c, clip_lo=lo, clip_hi=hi, act_dev=_ptr(act))
            return d, act
        return agree, make, given

    def smooth_target_action_group(self, members, *, noise_std=None, noise_clip=None, clip=(-1.0, 1.0), seed=0):
        """smooth_target_action for G target actors' outputs of ONE batch size and dtype, 1 <= G <= 8, in the two launches of one call
        (include/ptg_env.h: ptg_rsample_group with PTG_RS_SMOOTH); every member's actions are, bit for bit, what
        smooth_target_action gives for its arguments, and every member's counter advances by one.  members: a list of G dicts (mean,
        counter, and any of noise_std, noise_clip, clip, seed, out); noise_std, noise_clip, clip (a tuple) and seed here are one value
        for the members that do not name them, or a list with one per member.  No counter may serve two members.  Returns the list of G
        action tensors."""
        made = self._train_group("smooth_target_action_group", "smooth_target_action", members, ("mean", "counter", "noise_std", "noise_clip"), ("clip", "seed", "out"),
                                 dict(noise_std=noise_std, noise_clip=noise_clip, clip=clip, seed=seed), lambda who, kw: self._smooth_member(who, **kw))
        self._call("ptg_rsample_group", (_lib.PtgRs * len(made))(*[m[0] for m in made]), len(made))
        return [m[1] for m in made]

    # ------------------------------------------------------------------ the actor and entropy-coefficient losses and their gradients
    def actor_loss_workspace(self, batch):
        """the device scratch of actor_loss for a batch of this size (a uint8 tensor; reuse it across calls of up to that size)"""
        return self._loss_workspace("actor_loss", batch)

    def actor_loss(self, kind, q=None, log_prob=None, ent_coef=None, log_ent_coef=None, target_entropy=None, out=None, workspace=None):
        """Enqueue, on the current stream, the actor loss of SB3's SAC.train (kind "sac"), sb3_contrib's TQC.train ("tqc") or TD3.train
        ("td3"), and / or the entropy-coefficient loss ("ent_coef": that one alone), with their gradients (include/ptg_env.h:
        ptg_actor_loss, which states the arithmetic).
        "sac": q a list of K critic outputs on (obs, a_pi), [B] or [B, 1] each with any stride >= 1 (1 <= K <= 4).  "tqc": q a [B, K, Q]
        tensor or a list of K [B, Q] tensors as quantile_loss takes them.  "td3": q the first critic's output [B] / [B, 1]; no log_prob,
        no coefficient.  "sac" / "tqc" take log_prob [B] / [B, 1] contiguous in q's dtype and exactly one of ent_coef (a Python float, or
        a float64 device tensor of 1 element read when the kernel runs -- e.g. stats[4:5] of an earlier "ent_coef" call) and
        log_ent_coef (a float64 device tensor of 1 element).  target_entropy (a finite float; needs log_ent_coef): also emit the
        entropy-coefficient loss.  "ent_coef": log_prob, log_ent_coef and target_entropy, no q.
        Returns ActorLoss(stats float64 [8] = actor_loss, ent_coef_loss, mean log_prob, mean m, alpha as used, d ent_coef_loss / d
        log alpha, 0, 0; grad_q as q came (None for "ent_coef"); grad_log_prob shaped like log_prob (None for "td3" / "ent_coef");
        grad_log_ent_coef float64 [1] (None without target_entropy)).  out: an earlier result, reused by a captured call (its
        grad_log_prob and grad_log_ent_coef may be None: not written); workspace: actor_loss_workspace(B) or larger.  No synchronisation;
        a non-finite row makes the next sync() raise PtgError (PTG_E_NONFINITE)."""
        d, res, _ = self._actor_loss_member("actor_loss", kind, q=q, log_prob=log_prob, ent_coef=ent_coef, log_ent_coef=log_ent_coef, target_entropy=target_entropy,
                                            out=out, workspace=workspace)[1]()
        self._call("ptg_actor_loss", C.byref(d))
        return res

    def _actor_loss_member(self, who, kind, q=None, log_prob=None, ent_coef=None, log_ent_coef=None, target_entropy=None, out=None, workspace=None):
        """Every check of ONE actor-loss call, in actor_loss's order, for actor_loss and for each member of actor_loss_group; returns
        (agree, make, given) as _td_loss_member does, make() giving (the PtgAl, the ActorLoss, the workspace)"""
        torch = self._torch
        if kind not in ("sac", "tqc", "td3", "ent_coef"):
            raise ValueError(f"{who}: kind must be 'sac', 'tqc', 'td3' or 'ent_coef', got {kind!r}")
        floats = (torch.float32, torch.float64)
        only, td3 = kind == "ent_coef", kind == "td3"
        as_list = isinstance(q, (list, tuple))
        K, Q, dt, B, qs = 0, 1, floats, None, []
        if only:
            if q is not None:
                raise ValueError(f"{who}: kind 'ent_coef' reads no q")
        elif kind == "tqc":
            qs = self._quantile_views(who, "q", q, floats)
            (B, Q), K, dt = qs[0].shape, len(qs), (qs[0].dtype,)
            if not 1 <= Q <= _lib.QL_MAX_QUANTILES:
                raise ValueError(f"{who}: q needs 1 <= Q <= {_lib.QL_MAX_QUANTILES}, got Q = {Q}")
        else:
            if td3 and not as_list:
                q_list = [q]
            elif not as_list:
                raise TypeError(f"{who}: q must be a list of critic outputs for kind {kind!r}, got {type(q).__name__}")
            else:
                q_list = list(q)
            if not 1 <= len(q_list) <= (1 if td3 else _lib.TD_MAX_CRITICS):
                raise ValueError(f"{who}: q must hold {'one critic' if td3 else f'1 to {_lib.TD_MAX_CRITICS} critics'}, got {len(q_list)}")
            qs = _critic_columns(self, who, "q", q_list, floats)
            dt, (B,), K = (qs[0].dtype,), qs[0].shape, len(qs)
        if td3 and not (log_prob is None and ent_coef is None and log_ent_coef is None and target_entropy is None):
            raise ValueError(f"{who}: kind 'td3' takes q alone")
        if not td3 and log_prob is None:
            raise ValueError(f"{who}: kind {kind!r} needs log_prob")
        lp = check(self, who, "log_prob", _column(self, log_prob), dtypes=dt, shape=(B,), rule=contiguous, optional=True)
        if only:
            B, dt = lp.shape[0], (lp.dtype,)
        if B < 1:
            raise ValueError(f"{who}: an empty batch")
        if not td3 and (ent_coef is not None) + (log_ent_coef is not None) != 1:
            raise ValueError(f"{who}: kind {kind!r} takes exactly one of ent_coef and log_ent_coef")
        if (only or target_entropy is not None) and log_ent_coef is None:
            raise ValueError(f"{who}: the entropy-coefficient loss needs log_ent_coef")
        if only and target_entropy is None:
            raise ValueError(f"{who}: kind 'ent_coef' needs target_entropy")
        if target_entropy is not None and not np.isfinite(float(target_entropy)):
            raise ValueError(f"{who}: target_entropy must be finite, got {target_entropy}")
        ec = target_entropy is not None
        alpha_dev, alpha = _alpha_arg(self, who, ent_coef, log_ent_coef)
        g_q = gs = g_lp = g_la = None
        if out is not None:
            stats, g_q, g_lp, g_la = _out_tuple(self, who, out, ActorLoss)
            if only:
                if g_q is not None:
                    raise ValueError(f"{who}: out.grad_q given, but kind 'ent_coef' reads no q")
                gs = []
            elif kind == "tqc":
                if isinstance(g_q, (list, tuple)) != as_list:
                    raise ValueError(f"{who}: out.grad_q must be a {'list of ' + str(K) + ' tensors' if as_list else 'tensor'}, as q is")
                gs = self._quantile_views(who, "out.grad_q", g_q, dt, B, K, Q, exc=ValueError)
            else:
                g_list = [g_q] if td3 and not as_list else g_q
                if not isinstance(g_list, (list, tuple)) or len(g_list) != K:
                    raise ValueError(f"{who}: out.grad_q must be {'a tensor' if td3 and not as_list else f'a list of {K} tensors'}")
                gs = _critic_columns(self, who, "out.grad_q", g_list, dt, B, exc=ValueError)
            if g_lp is not None and (td3 or only):
                raise ValueError(f"{who}: out.grad_log_prob given, but kind {kind!r} has no entropy term")
            if g_la is not None and not ec:
                raise ValueError(f"{who}: out.grad_log_ent_coef given without target_entropy")
            check(self, who, "out.grad_log_prob", _column(self, g_lp), dtypes=dt, shape=(B,), rule=contiguous, optional=True, exc=ValueError)
            check(self, who, "out.grad_log_ent_coef", g_la, dtypes=(torch.float64,), shape=(1,), optional=True, exc=ValueError)
            _no_tensor_twice(who, list(gs) + qs + [x for x in (lp, g_lp) if x is not None], "out.grad_q, out.grad_log_prob, q and log_prob")
        self._take_workspace("actor_loss", B, workspace, who=who, fresh=False)
        agree = (("kind", kind), ("the number of critics", K), ("the number of quantiles", Q), ("the dtype", dt[0]), ("log_ent_coef given or not", log_ent_coef is not None),
                 ("target_entropy given or not", ec), ("the batch", B))
        theirs = None if out is None else (stats, g_q, gs, g_lp, g_la)
        given = ([] if out is None else [stats] + list(gs) + [t for t in (g_lp, g_la) if t is not None]) + ([] if workspace is None else [workspace])

        def make():
            ws = self._loss_workspace("actor_loss", B) if workspace is None else workspace
            g_q = gs = None
            if theirs is None:
                with torch.cuda.device(self.device):
                    mk = lambda shape, d=dt[0]: torch.empty(tuple(shape), dtype=d, device=self.device)
                    stats = mk((8,), torch.float64)
                    if kind == "tqc":
                        g_q, gs = self._fresh_like_quantiles(as_list, B, K, Q, dt[0])
                    elif not only:
                        g_list = [mk(t.shape) for t in (q if as_list else [q])]
                        gs, g_q = [_column(self, t) for t in g_list], (g_list if as_list else g_list[0])
                    g_lp = mk(log_prob.shape) if not (td3 or only) else None
                    g_la = mk((1,), torch.float64) if ec else None
            else:
                stats, g_q, gs, g_lp, g_la = theirs
            flags = (0 if td3 or only else _lib.AL_ENTROPY) | (_lib.AL_LOG_ALPHA if log_ent_coef is not None else 0) | (_lib.AL_ENT_COEF if ec else 0)
            d = _lib.PtgAl(kind=_lib.AL_ALPHA_ONLY if only else (_lib.AL_MIN if kind == "sac" else _lib.AL_MEAN), flags=flags, n_critics=K, n_quantiles=Q,
                           q_dtype=_out_code(torch, dt[0]), batch=B, logp_dev=_ptr(lp), alpha_dev=_ptr(alpha_dev), alpha=alpha,
                           target_entropy=float(target_entropy) if ec else 0.0, stats_dev=_ptr(stats), grad_logp_dev=_ptr(_column(self, g_lp)),
                           grad_log_alpha_dev=_ptr(g_la), ws_dev=_ptr(ws))
            for k in range(K):
                d.q_dev[k], d.q_s_n[k] = qs[k].data_ptr(), max(qs[k].stride(0), Q)
                d.grad_q_dev[k], d.g_s_n[k] = gs[k].data_ptr(), max(gs[k].stride(0), Q)
            return d, ActorLoss(stats, g_q, g_lp, g_la), ws
        return agree, make, given

    def actor_loss_group(self, kind, members, *, ent_coef=None, target_entropy=None):
        """actor_loss for G independent agents' batches of ONE batch size, 1 <= G <= 8, in exactly the launches of one actor_loss call
        (include/ptg_env.h: ptg_actor_loss_group).  Every member's result is, bit for bit, what actor_loss gives
        for its arguments.  members: a list of G dicts of actor_loss's arguments by name (any of q, log_prob, ent_coef, log_ent_coef,
        target_entropy, out, workspace, as the kind asks); ent_coef and target_entropy here are one value for the members that do not name
        them, or a list with one per member.  The members must agree in kind, K, Q, the dtype, whether log_ent_coef and target_entropy are
        given, and B; every scalar may differ.  No tensor may serve two members as an output or workspace.  Checked as actor_loss checks,
        member by member, the message behind "member i:"; nothing is allocated and the library is not touched before every check has
        passed.  Returns the list of G ActorLoss."""
        made = self._train_group("actor_loss_group", "actor_loss", members, (), ("q", "log_prob", "ent_coef", "log_ent_coef", "target_entropy", "out", "workspace"),
                                 dict(ent_coef=ent_coef, target_entropy=target_entropy), lambda who, kw: self._actor_loss_member(who, kind, **kw))
        self._call("ptg_actor_loss_group", (_lib.PtgAl * len(made))(*[m[0] for m in made]), len(made))      # made holds the workspaces until here
        return [m[1] for m in made]

    # ------------------------------------------------------------------ the inference forward of an MLP
    def mlp_workspace(self, batch, widths, keep_hidden=False):
        """bytes of device scratch mlp_forward needs for `batch` rows of a net with these layer widths: what ptg_mlp_workspace returns
        (include/ptg_env.h documents the layout), computed here so that the argument checks need no library"""
        batch, widths = _mlp_range("mlp_workspace", batch, widths)
        pitches = [_pitch(w) for w in widths[:-1]]
        return max(16, 4 * batch * (sum(pitches) if keep_hidden else 2 * max(pitches, default=0)))

    def _mlp_types(self, who, x, x2, weights, biases, first=(), grad_weights=None, grad_biases=None):
        """the TypeError half of _mlp_net: what every value is.  A group runs it over all its networks before the other half of any."""
        torch = self._torch
        f32 = (torch.float32,)
        if not isinstance(weights, (list, tuple)) or not isinstance(biases, (list, tuple)):
            raise TypeError(f"{who}: weights and biases must be lists of tensors, got {type(weights).__name__} and {type(biases).__name__}")
        if (grad_weights is None) != (grad_biases is None):
            raise TypeError(f"{who}: grad_weights and grad_biases go together")
        if grad_weights is not None and (not isinstance(grad_weights, (list, tuple)) or not isinstance(grad_biases, (list, tuple))):
            raise TypeError(f"{who}: grad_weights and grad_biases must be lists, got {type(grad_weights).__name__} and {type(grad_biases).__name__}")
        named = list(first) + [("x", x), ("x2", x2)] + [(f"weights[{l}]", w) for l, w in enumerate(weights)] + [(f"biases[{l}]", b) for l, b in enumerate(biases)]
        for name, t in named:                                # TypeError first: what every value is
            if not (t is None and name == "x2") and (not torch.is_tensor(t) or t.dtype not in f32):
                check(self, who, name, t, dtypes=f32)

    def _mlp_net(self, who, x, x2, weights, biases, hidden_activation, out_activation, route=None, first=(), grad_weights=None, grad_biases=None,
                 typed=False, split=False):
        """The checks of a net that mlp_forward and mlp_backward share, in their one order: TypeError for what every value is (`first`:
        the (name, tensor) pairs the caller puts before x; typed: the caller has run _mlp_types already), then ValueError for the names,
        the counts, x, x2 and layer by layer the weights, the biases and, where given, the gradients.  split: x is [B, 16] split
        observation rows and F1 the width of the flat row they stand for on this engine (policy_split.flat_columns), which the first
        weight's fan-in must match.  Returns B, F1, F2, the widths and fill(out, workspace, flags), which makes the call's ptg_mlp
        (split: with MLP_SPLIT_INPUT among its flags)."""
        torch = self._torch
        f32 = (torch.float32,)
        acts = {"relu": _lib.MLP_RELU, "tanh": _lib.MLP_TANH, None: _lib.MLP_NONE}
        if not typed:
            self._mlp_types(who, x, x2, weights, biases, first=first, grad_weights=grad_weights, grad_biases=grad_biases)
        if hidden_activation not in ("relu", "tanh"):
            raise ValueError(f"{who}: hidden_activation must be 'relu' or 'tanh', got {hidden_activation!r}")
        if out_activation not in acts:
            raise ValueError(f"{who}: out_activation must be None, 'relu' or 'tanh', got {out_activation!r}")
        if route not in (None, "narrow", "wide"):
            raise ValueError(f"{who}: _route must be None, 'narrow' or 'wide', got {route!r}")
        n = len(weights)
        if not 1 <= n <= _lib.MLP_MAX_LAYERS or len(biases) != n:
            raise ValueError(f"{who}: 1 to {_lib.MLP_MAX_LAYERS} layers with one bias each, got {n} weights and {len(biases)} biases")
        if grad_weights is not None and (len(grad_weights) != n or len(grad_biases) != n):
            raise ValueError(f"{who}: grad_weights and grad_biases must have {n} entries, got {len(grad_weights)} and {len(grad_biases)}")
        check(self, who, "x", x, dtypes=f32, shape=(None, 16 if split else None), rule=rows)
        B, F1 = x.shape
        if split:
            from .policy_split import flat_columns
            F1 = flat_columns("mod" if self.consts["raw_modified"] else "raw", int(self.consts["price_ahead"]))[1]
        check(self, who, "x2", x2, dtypes=f32, shape=(B, None), rule=rows, optional=True)
        F2 = 0 if x2 is None else x2.shape[1]
        if B < 1 or F1 < 1 or (x2 is not None and F2 < 1):
            raise ValueError(f"{who}: an empty batch or an empty input piece: x {tuple(x.shape)}" + ("" if x2 is None else f", x2 {tuple(x2.shape)}"))
        fan_in, widths = F1 + F2, []
        for l in range(n):
            if not 1 <= fan_in <= _lib.MLP_MAX_WIDTH:
                raise ValueError(f"{who}: the fan-in of layer {l} is {fan_in}, outside [1, {_lib.MLP_MAX_WIDTH}]")
            check(self, who, f"weights[{l}]", weights[l], dtypes=f32, shape=(None, fan_in), rule=rows)
            fan_out = weights[l].shape[0]
            check(self, who, f"biases[{l}]", biases[l], dtypes=f32, shape=(fan_out,), rule=contiguous)
            if grad_weights is not None:
                if (grad_weights[l] is None) != (grad_biases[l] is None):
                    raise ValueError(f"{who}: grad_weights[{l}] and grad_biases[{l}] go together")
                check(self, who, f"grad_weights[{l}]", grad_weights[l], dtypes=f32, shape=(fan_out, fan_in), rule=rows, optional=True, exc=ValueError)
                check(self, who, f"grad_biases[{l}]", grad_biases[l], dtypes=f32, shape=(fan_out,), rule=contiguous, optional=True, exc=ValueError)
            fan_in = fan_out
            widths.append(fan_in)
        if not 1 <= fan_in <= _lib.MLP_MAX_WIDTH:
            raise ValueError(f"{who}: the output width is {fan_in}, outside [1, {_lib.MLP_MAX_WIDTH}]")

        def fill(out, workspace, flags):
            d = _lib.PtgMlp(batch=B, n_layers=n, flags=flags | (_lib.MLP_SPLIT_INPUT if split else 0), hidden_act=acts[hidden_activation], out_act=acts[out_activation], f1=F1, f2=F2,
                            x_dev=_ptr(x), x_s_n=_row_stride(x), x2_dev=_ptr(x2), x2_s_n=0 if x2 is None else _row_stride(x2), out_dev=_ptr(out),
                            out_s_n=_row_stride(out), ws_dev=_ptr(workspace), ws_bytes=workspace.numel())
            for l in range(n):
                d.w_dev[l], d.w_s_n[l], d.b_dev[l], d.width[l] = weights[l].data_ptr(), _row_stride(weights[l]), biases[l].data_ptr(), widths[l]
            return d

        return B, F1, F2, widths, fill

    def _mlp_forward_net(self, who, x, x2, weights, biases, hidden_activation, out_activation, out, workspace, keep_hidden, route=None, typed=False,
                         split=False):
        """Every check of ONE network's forward, for mlp_forward (who "mlp_forward") and for mlp_group_forward (who "mlp_group_forward: net i",
        typed): _mlp_net, then out, then the workspace.  Returns B, the widths, the workspace's bytes and _mlp_net's fill."""
        B, _, _, widths, fill = self._mlp_net(who, x, x2, weights, biases, hidden_activation, out_activation, route=route, typed=typed, split=split)
        check(self, who, "out", out, dtypes=(self._torch.float32,), shape=(B, widths[-1]), rule=rows, optional=True, exc=ValueError)
        need = self.mlp_workspace(B, widths, keep_hidden)
        if workspace is not None:
            _workspace_arg(self, who, f"workspace (mlp_workspace({B}, {widths}, {bool(keep_hidden)}))", workspace, need)
        return B, widths, need, fill

    def _mlp_backward_net(self, who, grad_out, x, x2, weights, biases, hidden_activation, out_activation, out, workspace, grad_weights, grad_biases, grad_x, grad_x2,
                          backward_workspace, typed=False, split=False):
        """Every check of ONE network's backward, for mlp_backward and for mlp_group_backward as _mlp_forward_net is for the forwards.
        Returns B, the widths, the backward workspace's bytes, _mlp_net's fill and the tensors the network writes."""
        f32 = (self._torch.float32,)
        B, F1, F2, widths, fill = self._mlp_net(who, x, x2, weights, biases, hidden_activation, out_activation, first=[("grad_out", grad_out)],
                                                grad_weights=grad_weights, grad_biases=grad_biases, typed=typed, split=split)
        check(self, who, "grad_out", grad_out, dtypes=f32, shape=(B, widths[-1]), rule=rows)
        check(self, who, "out", out, dtypes=f32, shape=(B, widths[-1]), rule=rows, exc=ValueError)
        _workspace_arg(self, who, f"workspace (mlp_workspace({B}, {widths}, True))", workspace, self.mlp_workspace(B, widths, True), "the forward with keep_hidden needs")
        if split and grad_x is not None:
            raise ValueError(f"{who}: grad_x with split=True: an observation has no gradient")
        check(self, who, "grad_x", grad_x, dtypes=f32, shape=(B, F1), rule=rows, optional=True, exc=ValueError)
        if grad_x2 is not None and x2 is None:
            raise ValueError(f"{who}: grad_x2 without x2")
        check(self, who, "grad_x2", grad_x2, dtypes=f32, shape=(B, F2), rule=rows, optional=True, exc=ValueError)
        need = self.mlp_backward_workspace(B, widths)
        if backward_workspace is not None:
            _workspace_arg(self, who, f"backward_workspace (mlp_backward_workspace({B}, {widths}))", backward_workspace, need)
        written = [t for t in (list(grad_weights or []) + list(grad_biases or []) + [grad_x, grad_x2, backward_workspace]) if t is not None]
        return B, widths, need, fill, written

    def mlp_forward(self, x, weights, biases, hidden_activation="relu", out_activation=None, x2=None, out=None, workspace=None, keep_hidden=False,
                    _route=None, split=False):
        """Enqueue, on the current stream, the forward pass of an MLP without autograd: one fused launch per layer (include/ptg_env.h:
        ptg_mlp_forward, which states the arithmetic -- per unit a float32 fmaf chain from the bias over ascending k, then the activation).
        x [B, F1] float32 with unit column stride and a row stride >= F1 (a column slice of a wider tensor fits); x2 [B, F2] likewise, or
        None: the net reads th.cat([x, x2], 1) without the cat.  weights[l] [out_l, in_l] float32 in torch's Linear.weight layout with
        unit column stride, biases[l] [out_l] contiguous; in_0 = F1 + F2, in_l = out_(l-1); 1 to 10 layers, every width and the fan-in in
        [1, 1024].  hidden_activation "relu" | "tanh" after every layer but the last, out_activation None | "relu" | "tanh" after the last.
        out: [B, O] float32 with unit column stride and a row stride >= O, allocated when None.  workspace: a contiguous uint8 tensor
        of at least mlp_workspace(B, widths, keep_hidden) bytes, 4-byte aligned, allocated when None.  keep_hidden: the post-activation
        hidden layers stay in the workspace and are returned as views into it.  Returns MlpOut(out, hidden): hidden a tuple of n - 1
        [B, width_l] views, or None.  No synchronisation and, with out= and workspace=, no allocation; a -0 result may come out as +0.
        `_route` ("narrow" | "wide") forces one tile route in every layer: for tests and measurements, the bits do not depend on it.
        split: x is [B, 16] split observation rows (obs_layout="split"; row stride >= 16) and the first layer reads the flat row they
        stand for, rebuilt from the engine's market series while it loads (include/ptg_env.h: PTG_MLP_SPLIT_INPUT; DESIGN.md section
        21): weights[0] has the flat row's width (policy_split.flat_columns of the engine's raw_modified and price_ahead) plus F2 input
        columns, and the result has the bits of the same call on policy_split.flat_rows_from_split(x).  A row whose hour or day index
        is no integer inside the series gives NaN outputs, and the next sync() raises PTG_E_INDEX."""
        net = self._mlp_forward_net("mlp_forward", x, x2, weights, biases, hidden_activation, out_activation, out, workspace, keep_hidden, route=_route,
                                    split=split)
        flags = (_lib.MLP_KEEP_HIDDEN if keep_hidden else 0) | {None: 0, "narrow": _lib.MLP_NARROW, "wide": _lib.MLP_WIDE}[_route]
        d, res, workspace = _mlp_fwd_desc(self, net, out, workspace, keep_hidden, flags)
        self._call("ptg_mlp_forward", C.byref(d))
        return res

    # ------------------------------------------------------------------ the backward pass of an MLP
    def mlp_backward_workspace(self, batch, widths):
        """bytes of device scratch mlp_backward needs: what ptg_mlp_backward_workspace returns (two alternating [batch, P(widest width)]
        float32 buffers for dz), computed here so that the argument checks need no library"""
        batch, widths = _mlp_range("mlp_backward_workspace", batch, widths)
        return 8 * batch * max(_pitch(w) for w in widths)

    def mlp_backward(self, grad_out, x, weights, biases, out, workspace, hidden_activation="relu", out_activation=None, x2=None, grad_weights=None,
                     grad_biases=None, grad_x=None, grad_x2=None, backward_workspace=None, accumulate=False, split=False):
        """Enqueue, on the current stream, the backward pass of the MLP whose forward was mlp_forward(x, weights, biases, ..., out=out,
        workspace=workspace, keep_hidden=True) with the same arguments (include/ptg_env.h: ptg_mlp_backward, which states the arithmetic:
        float32 fmaf chains, dx over ascending units, dW and db over ascending rows).  grad_out [B, O] float32, unit column stride, a row
        stride >= O.  x, x2, weights, biases, out, workspace: what the forward was given and returned, unchanged since.  grad_weights /
        grad_biases: lists of n tensors shaped like the parameters (grad_weights[l] may have a row stride above its fan-in), an entry None
        in both freezes that layer; both None: no parameter gradients.  grad_x [B, F1] / grad_x2 [B, F2]: each optional; with neither, the
        first layer's input gradient is not computed.  backward_workspace: contiguous uint8, >= mlp_backward_workspace(B, widths) bytes,
        4-byte aligned, allocated when None.  accumulate: the parameter gradients are added to in place, continuing each element's chain
        over the rows.  Nothing but backward_workspace is allocated; no synchronisation.  Returns the backward workspace (dz of layers 0
        and 1 stay in it: include/ptg_env.h has the layout).  split: as in the forward, which must have had it too; the first layer's
        weight and bias gradients read the rebuilt flat row, and grad_x must be None: an observation has no gradient."""
        net = self._mlp_backward_net("mlp_backward", grad_out, x, x2, weights, biases, hidden_activation, out_activation, out, workspace, grad_weights, grad_biases,
                                     grad_x, grad_x2, backward_workspace, split=split)
        _no_tensor_twice("mlp_backward", net[4], "grad_weights, grad_biases, grad_x, grad_x2 and backward_workspace")
        d, backward_workspace = _mlp_bwd_desc(self, net, grad_out, out, workspace, grad_weights, grad_biases, grad_x, grad_x2, backward_workspace, accumulate)
        self._call("ptg_mlp_backward", C.byref(d))
        return backward_workspace

    # ------------------------------------------------------------------ MLPs of equal depth in the launches of one
    def _mlp_group(self, who, weights, biases):
        """G of a grouped call, from its lists of lists"""
        if not isinstance(weights, (list, tuple)) or not isinstance(biases, (list, tuple)):
            raise TypeError(f"{who}: weights and biases must be lists with one list of tensors per network, got {type(weights).__name__} and {type(biases).__name__}")
        G = len(weights)
        if not 1 <= G <= _lib.MLP_GROUP_MAX:
            raise ValueError(f"{who}: 1 to {_lib.MLP_GROUP_MAX} networks, got {G}")
        if len(biases) != G:
            raise ValueError(f"{who}: biases must have one entry per network, {G}, got {len(biases)}")
        return G

    def _mlp_group_agree(self, who, nets):
        """nets: what _mlp_forward_net or _mlp_backward_net returned per network; batch and depth must agree with network 0's"""
        for i, net in enumerate(nets):
            if net[0] != nets[0][0]:
                raise ValueError(f"{who}: nets 0 and {i} disagree in the batch: {nets[0][0]} and {net[0]} rows")
            if len(net[1]) != len(nets[0][1]):
                raise ValueError(f"{who}: nets 0 and {i} disagree in depth: {len(nets[0][1])} and {len(net[1])} layers")

    def mlp_group_forward(self, xs, weights, biases, hidden_activation="relu", out_activation=None, x2s=None, outs=None, workspaces=None, keep_hidden=False,
                          split=False):
        """mlp_forward for G networks, 1 <= G <= 8, of equal depth, activations and batch in ONE launch per layer (include/ptg_env.h:
        ptg_mlp_group_forward): twin critics, critics and their targets, a policy and a value net.  Every network's result is, bit for
        bit, what mlp_forward gives for its arguments.  xs: a list of G tensors [B, F1_i], or one tensor that every network reads;
        weights / biases: lists of G lists as mlp_forward takes them (widths may differ, the depth may not); x2s, outs, workspaces: None,
        or lists of G entries in which None stands where mlp_forward allows None.  Networks may share inputs and even weights; no tensor
        may serve two of the outs and workspaces.  The arguments are checked as mlp_forward checks them: TypeError for what the values
        of all networks are first, then ValueError network by network, the message behind "net i:".  split: every network's x holds
        split observation rows, as in mlp_forward.  Returns a list of G MlpOut."""
        who = "mlp_group_forward"
        G = self._mlp_group(who, weights, biases)
        xs, x2s = _per_net(who, "xs", xs, G, share=True), _per_net(who, "x2s", x2s, G, optional=True)
        outs, workspaces = _per_net(who, "outs", outs, G, optional=True), _per_net(who, "workspaces", workspaces, G, optional=True)
        for i in range(G):
            self._mlp_types(f"{who}: net {i}", xs[i], x2s[i], weights[i], biases[i])
        nets = [self._mlp_forward_net(f"{who}: net {i}", xs[i], x2s[i], weights[i], biases[i], hidden_activation, out_activation, outs[i], workspaces[i], keep_hidden,
                                      typed=True, split=split) for i in range(G)]
        self._mlp_group_agree(who, nets)
        _no_tensor_twice(who, [t for t in outs + workspaces if t is not None], "outs and workspaces")
        made = [_mlp_fwd_desc(self, nets[i], outs[i], workspaces[i], keep_hidden, _lib.MLP_KEEP_HIDDEN if keep_hidden else 0) for i in range(G)]
        self._call("ptg_mlp_group_forward", (_lib.PtgMlp * G)(*[m[0] for m in made]), G)      # made holds the workspaces until here
        return [m[1] for m in made]

    def mlp_group_backward(self, grad_outs, xs, weights, biases, outs, workspaces, hidden_activation="relu", out_activation=None, x2s=None, grad_weights=None,
                           grad_biases=None, grad_xs=None, grad_x2s=None, backward_workspaces=None, accumulate=False, split=False):
        """mlp_backward for the G networks of an mlp_group_forward(..., keep_hidden=True) call, in the launches of ONE network's backward
        (include/ptg_env.h: ptg_mlp_group_backward); every network's gradients are, bit for bit, what mlp_backward gives for its
        arguments.  grad_outs, outs, workspaces: lists of G; xs as in the forward; x2s, grad_weights, grad_biases, grad_xs, grad_x2s,
        backward_workspaces: None or lists of G entries, each what mlp_backward takes for that network (None in grad_weights[i] and
        grad_biases[i]: no parameter gradients for network i; a None inside them freezes that layer of that network; grad_xs[i] and
        grad_x2s[i] each optional).  A weight-gradient launch is enqueued for a layer when any network wants it, the first layer's
        input-gradient launch when any network wants a grad_x or grad_x2.  The gradient of an input that several networks share is NOT
        summed: each network writes its own grad_xs[i].  No tensor may serve two of the outputs.  Checked as mlp_group_forward checks.
        split: as in mlp_backward, for every network: every grad_xs[i] must be None.
        Returns the list of backward workspaces."""
        who = "mlp_group_backward"
        G = self._mlp_group(who, weights, biases)
        xs, x2s = _per_net(who, "xs", xs, G, share=True), _per_net(who, "x2s", x2s, G, optional=True)
        grad_outs, outs, workspaces = _per_net(who, "grad_outs", grad_outs, G), _per_net(who, "outs", outs, G), _per_net(who, "workspaces", workspaces, G)
        grad_weights, grad_biases = _per_net(who, "grad_weights", grad_weights, G, optional=True), _per_net(who, "grad_biases", grad_biases, G, optional=True)
        grad_xs, grad_x2s = _per_net(who, "grad_xs", grad_xs, G, optional=True), _per_net(who, "grad_x2s", grad_x2s, G, optional=True)
        bws = _per_net(who, "backward_workspaces", backward_workspaces, G, optional=True)
        for i in range(G):
            self._mlp_types(f"{who}: net {i}", xs[i], x2s[i], weights[i], biases[i], first=[("grad_out", grad_outs[i])], grad_weights=grad_weights[i],
                            grad_biases=grad_biases[i])
        nets = [self._mlp_backward_net(f"{who}: net {i}", grad_outs[i], xs[i], x2s[i], weights[i], biases[i], hidden_activation, out_activation, outs[i], workspaces[i],
                                       grad_weights[i], grad_biases[i], grad_xs[i], grad_x2s[i], bws[i], typed=True, split=split) for i in range(G)]
        self._mlp_group_agree(who, nets)
        _no_tensor_twice(who, [t for net in nets for t in net[4]], "grad_weights, grad_biases, grad_xs, grad_x2s and backward_workspaces")
        made = [_mlp_bwd_desc(self, nets[i], grad_outs[i], outs[i], workspaces[i], grad_weights[i], grad_biases[i], grad_xs[i], grad_x2s[i], bws[i], accumulate)
                for i in range(G)]
        self._call("ptg_mlp_group_backward", (_lib.PtgMlpBwd * G)(*[d for d, _ in made]), G)
        return [w for _, w in made]

    # ------------------------------------------------------------------ the optimiser step behind loss.backward()
    def optim_chunk(self):
        """elements per chunk of the optimiser kernels (one workgroup each)"""
        return int(self._L.ptg_optim_chunk())

    def optim_plan(self, params, grads, kind, targets=None, state=None):
        """Check the tensor lists of one optimiser and build what optim_step needs (include/ptg_env.h: ptg_optim_step): params, grads
        (None for kind "polyak") and targets (optional) are lists of contiguous tensors of ONE float dtype (float32 or float64) on the
        engine's device, grads[k] and targets[k] shaped like params[k]; a parameter may be a view into a flat buffer at any element
        offset.  kind: "adam" | "rmsprop" | "polyak".  Allocates the zeroed state tensors (state: an earlier plan of the same
        parameters whose state is taken over instead -- the gradients moved), the device scalars {t, beta1^t, beta2^t} and the total
        norm, the scratch, and uploads the tensor and chunk tables.  Returns an OptimPlan; it keeps every tensor alive.  Not for use
        under stream capture (it allocates and copies)."""
        torch = self._torch
        who = "optim_plan"
        if kind not in ("adam", "rmsprop", "polyak"):
            raise ValueError(f"{who}: kind must be 'adam', 'rmsprop' or 'polyak', got {kind!r}")
        polyak = kind == "polyak"
        params = list(params)
        grads = None if grads is None else list(grads)
        targets = None if targets is None else list(targets)
        floats = (torch.float32, torch.float64)
        for k, p in enumerate(params):                      # TypeError first: what every value is
            if not torch.is_tensor(p) or p.dtype not in floats:
                check(self, who, f"params[{k}]", p, dtypes=floats)
        dt = (params[0].dtype,) if params else floats
        lists = [("params", params), ("grads", grads), ("targets", targets)]
        if state is not None:
            lists += [(name, xs) for name, xs in (("state.state1", state.state1), ("state.state2", state.state2)) if xs]
        for name, xs in lists:
            for k, x in enumerate(xs or ()):
                if x is None and name == "grads":
                    continue                                # refused below, as a ValueError
                if not torch.is_tensor(x) or x.dtype not in dt:
                    check(self, who, f"{name}[{k}]", x, dtypes=dt)
        if not params:
            raise ValueError(f"{who}: an empty parameter list")
        if polyak and grads is not None:
            raise ValueError(f"{who}: kind 'polyak' takes no gradients")
        if not polyak and grads is None:
            raise ValueError(f"{who}: kind {kind!r} needs the gradients")
        if polyak and targets is None:
            raise ValueError(f"{who}: kind 'polyak' needs targets")
        for name, xs in lists[1:]:
            if xs is not None and len(xs) != len(params):
                raise ValueError(f"{who}: {len(params)} parameters but {len(xs)} {name}")
        for k, p in enumerate(params):
            check(self, who, f"params[{k}]", p, dtypes=dt, rule=contiguous)
            if p.numel() < 1:
                raise ValueError(f"{who}: params[{k}] is empty")
            for name, xs in lists[1:]:
                if xs is None:
                    continue
                if xs[k] is None:
                    raise ValueError(f"{who}: params[{k}] has no gradient (torch.optim skips such a parameter; here every parameter of the plan takes the step)")
                check(self, who, f"{name}[{k}]", xs[k], dtypes=dt, shape=tuple(p.shape), rule=contiguous)
        C_ = self.optim_chunk()
        n_chunks = sum((p.numel() + C_ - 1) // C_ for p in params)
        nbytes = self._L.ptg_optim_workspace(n_chunks)
        if nbytes < 0:
            raise ValueError(f"{who}: {n_chunks} chunks of {C_} elements are more than one launch takes")
        plan = OptimPlan()
        plan.kind, plan.dtype, plan.params, plan.grads, plan.targets, plan.n_chunks = kind, params[0].dtype, params, grads, targets, n_chunks
        with torch.cuda.device(self.device):
            if state is not None:
                plan.state1, plan.state2, plan.state, plan.norm = state.state1, state.state2, state.state, state.norm
            else:
                plan.state1 = [] if polyak else [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in params]
                plan.state2 = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in params] if kind == "adam" else []
                plan.state = torch.tensor([0.0, 1.0, 1.0, 0.0], dtype=torch.float64).to(self.device)
                plan.norm = torch.zeros(1, dtype=torch.float64, device=self.device)
            ptr = lambda xs, k: xs[k].data_ptr() if xs else 0
            tab = np.array([[p.data_ptr(), ptr(grads, k), ptr(plan.state1, k), ptr(plan.state2, k), ptr(targets, k), p.numel()]
                            for k, p in enumerate(params)], dtype=np.int64)
            spans = np.array([[k, off] for k, p in enumerate(params) for off in range(0, p.numel(), C_)], dtype=np.int64)
            plan.tensors_dev = torch.from_numpy(tab).to(self.device)
            plan.chunks_dev = torch.from_numpy(spans).to(self.device)
            plan.workspace = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        plan.grad_ptrs = None if grads is None else [g.data_ptr() for g in grads]
        return plan

    def _optim_desc(self, plan, kind, flags):
        return _lib.PtgOptim(kind=kind, flags=flags, dtype=_out_code(self._torch, plan.dtype), n_tensors=len(plan.params), n_chunks=plan.n_chunks,
                             tensors_dev=_ptr(plan.tensors_dev), chunks_dev=_ptr(plan.chunks_dev), ws_dev=_ptr(plan.workspace))

    def optim_step(self, plan, lr, betas=(0.9, 0.999), eps=1e-8, alpha=0.99, max_grad_norm=None, tau=None, zero_grad=False):
        """Enqueue, on the current stream, ONE step of every parameter of the plan (include/ptg_env.h: ptg_optim_step, which states the
        arithmetic): clip_grad_norm_(max_grad_norm) unless it is None, torch.optim.Adam (plan kind "adam": betas, eps) or RMSprop
        ("rmsprop": alpha, eps; no momentum, not centered), SB3's polyak_update(params, targets, tau) when the plan has targets, and
        zero_grad(set_to_none=False).  lr: a Python float, kept by a captured call, or a float64 device tensor of 1 element, read when
        the kernel runs.  Three launches (two without clipping) whatever the number of tensors, no synchronisation, no allocation:
        the call may be captured and replayed, and every replay takes the next step t + 1.  plan.norm holds the total norm afterwards.
        A non-finite total norm (without clipping: gradient element) makes the next sync() raise PtgError with code PTG_E_NONFINITE."""
        self._call("ptg_optim_step", C.byref(self._optim_step_member("optim_step", plan, lr, betas, eps, alpha, max_grad_norm, tau, zero_grad)))

    def _optim_step_member(self, who, plan, lr, betas, eps, alpha, max_grad_norm, tau, zero_grad):
        """every check of ONE optim_step call, in its order, for optim_step and for each member of optim_step_group -> its PtgOptim"""
        torch = self._torch
        if not isinstance(plan, OptimPlan):
            raise TypeError(f"{who}: plan must be an OptimPlan (optim_plan()), got {type(plan).__name__}")
        if torch.is_tensor(lr):
            check(self, who, "a tensor lr", lr, dtypes=(torch.float64,), numel=1)
        else:
            lr = float(lr)
        if plan.kind == "polyak":
            raise ValueError(f"{who}: a 'polyak' plan has no optimiser (polyak_update takes it)")
        if not torch.is_tensor(lr) and not (lr >= 0.0 and np.isfinite(lr)):
            raise ValueError(f"{who}: lr must be finite and >= 0, got {lr}")
        b1, b2 = float(betas[0]), float(betas[1])
        if plan.kind == "adam" and not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError(f"{who}: betas must be in [0, 1), got {betas}")
        if not (float(eps) >= 0.0 and np.isfinite(float(eps))):
            raise ValueError(f"{who}: eps must be finite and >= 0, got {eps}")
        if not (float(alpha) >= 0.0 and np.isfinite(float(alpha))):
            raise ValueError(f"{who}: alpha must be finite and >= 0, got {alpha}")
        if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:
            raise ValueError(f"{who}: max_grad_norm must be >= 0 (or None), got {max_grad_norm}")
        if plan.targets is not None and tau is None:
            raise ValueError(f"{who}: a plan with targets needs tau")
        if plan.targets is None and tau is not None:
            raise ValueError(f"{who}: tau given, but the plan has no targets")
        if tau is not None and not 0.0 <= float(tau) <= 1.0:
            raise ValueError(f"{who}: tau must be in [0, 1], got {tau}")
        flags = (_lib.OPTIM_CLIP if max_grad_norm is not None else 0) | (_lib.OPTIM_TARGETS if plan.targets is not None else 0) | \
                (_lib.OPTIM_ZERO_GRAD if zero_grad else 0)
        d = self._optim_desc(plan, _lib.OPTIM_ADAM if plan.kind == "adam" else _lib.OPTIM_RMSPROP, flags)
        d.state_dev, d.norm_dev = _ptr(plan.state), _ptr(plan.norm)
        if torch.is_tensor(lr):
            d.lr_dev = _ptr(lr)
        else:
            d.lr = lr
        d.beta1, d.beta2, d.eps, d.alpha = b1, b2, float(eps), float(alpha)
        d.tau = float(tau) if tau is not None else 0.0
        d.max_norm = float(max_grad_norm) if max_grad_norm is not None else 0.0
        return d

    def optim_step_group(self, plans, lrs, betas=(0.9, 0.999), eps=1e-8, alpha=0.99, max_grad_norm=None, tau=None, zero_grad=False):
        """optim_step for G plans of ONE kind and dtype, 1 <= G <= 8, in exactly the launches of one optim_step call -- three, two without
        clipping, whatever G is (include/ptg_env.h: ptg_optim_step_group).  Every member's parameters, states,
        targets, zeroed gradients, step count and plan.norm are, bit for bit, what optim_step gives for its arguments.  plans: a list
        of G OptimPlans; lrs, betas, eps, alpha, max_grad_norm, tau: each a list with one entry per member, or one value for all (lrs:
        floats and float64 device tensors may be mixed; betas: a pair for all, or a list of G pairs).  The members must agree in the
        plan's kind and dtype, in clipping or not (max_grad_norm None or not), in having targets or not, and in zero_grad (ValueError,
        which names the two members); no plan may be given twice.  Checked as optim_step checks, member by member, the message behind
        "member i:".  No synchronisation, no allocation: the call may be captured and replayed.
        Cost (profiles/train_group_cost.txt; DESIGN.md section 26, whose one condition held at every shape): see DeviceOptimizerGroup's docstring."""
        who = "optim_step_group"
        if not isinstance(plans, (list, tuple)):
            raise TypeError(f"{who}: plans must be a list of OptimPlans, got {type(plans).__name__}")
        G = len(plans)
        if not 1 <= G <= _lib.TRAIN_GROUP_MAX:
            raise ValueError(f"{who}: 1 to {_lib.TRAIN_GROUP_MAX} members, got {G}")

        def per(name, x, one=lambda v: not isinstance(v, (list, tuple))):
            if one(x):
                return [x] * G
            if len(x) != G:
                raise ValueError(f"{who}: {name} must have one entry per member, {G}, or be one value for all; got {len(x)}")
            return list(x)
        lrs, eps, alpha, mgn, tau = per("lrs", lrs), per("eps", eps), per("alpha", alpha), per("max_grad_norm", max_grad_norm), per("tau", tau)
        betas = per("betas", betas, one=lambda v: len(v) == 2 and not isinstance(v[0], (list, tuple)))
        descs = [self._optim_step_member(f"{who}: member {i}", plans[i], lrs[i], betas[i], eps[i], alpha[i], mgn[i], tau[i], zero_grad) for i in range(G)]
        for i in range(1, G):
            for name, a, b in (("the plan's kind", plans[0].kind, plans[i].kind), ("the dtype", plans[0].dtype, plans[i].dtype),
                               ("clipping (max_grad_norm None or not)", mgn[0] is not None, mgn[i] is not None),
                               ("having targets", plans[0].targets is not None, plans[i].targets is not None)):
                if a != b:
                    raise ValueError(f"{who}: members 0 and {i} disagree in {name}: {a} and {b}")
        if len({id(p) for p in plans}) != G:
            raise ValueError(f"{who}: a plan is given twice; every member steps its own parameters")
        _no_tensor_twice(who, [t for p in plans for t in (p.state, p.norm, p.workspace)], "the plans' state, norm and workspace")
        self._call("ptg_optim_step_group", (_lib.PtgOptim * G)(*descs), G)

    def polyak_update(self, params, targets, tau, plan=None):
        """Enqueue, on the current stream, SB3's polyak_update(params, targets, tau) for lists that no optimiser steps -- DQN's hard
        update with tau = 1, batch-norm statistics: target = (1 - tau) * target + tau * param in ONE launch.  plan: the OptimPlan of an
        earlier call on the same lists (returned here), which makes the call free of allocation and fit for capture; without it the
        lists are checked and a plan is built first.  Returns the plan."""
        who = "polyak_update"
        if plan is not None and (not isinstance(plan, OptimPlan) or plan.kind != "polyak"):
            raise TypeError(f"{who}: plan must be the OptimPlan an earlier polyak_update returned")
        if not 0.0 <= float(tau) <= 1.0:
            raise ValueError(f"{who}: tau must be in [0, 1], got {tau}")
        if plan is None:
            plan = self.optim_plan(params, None, "polyak", targets=targets)
        elif params is not None and ([p.data_ptr() for p in params] != [p.data_ptr() for p in plan.params] or
                                     [q.data_ptr() for q in targets] != [q.data_ptr() for q in plan.targets]):
            raise ValueError(f"{who}: the plan was built for other tensors")
        d = self._optim_desc(plan, _lib.OPTIM_POLYAK, 0)
        d.tau = float(tau)
        self._call("ptg_optim_step", C.byref(d))
        return plan
