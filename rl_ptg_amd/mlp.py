"""DeviceMLP: the inference forward of a torch MLP as one fused launch per layer (HipEngine.mlp_forward, include/ptg_env.h:
ptg_mlp_forward, which states the arithmetic).  TrainMLP, below: the training forward and the backward pass under autograd.
DeviceMLPGroup and TrainMLPGroup, at the end: several networks of equal depth in the launches of one.

    policy = DeviceMLP(engine, q_net, batch=engine.n)                 # an nn.Sequential of Linear / ReLU / Tanh, as SB3's create_mlp returns
    logits = policy(obs)                                              # no autograd graph, no allocation, no synchronisation
    mean = DeviceMLP(engine, [latent_pi, mu], batch=256)              # a list chains: the trunk, then a head
    q_next = DeviceMLP(engine, target_qf, batch=256)(next_obs, x2=next_actions)      # th.cat([obs, action], 1) without the cat

The parameters are held BY REFERENCE, never copied: what DeviceOptimizer.step() and polyak_update write in place is what the next call,
and the next replay of a captured call, reads.  Output and workspace are allocated once, for `batch` rows; a call with fewer rows
returns the first rows of the output tensor, and every call overwrites it.

obs="split" (all four classes): x is the [B, 16] rows of an engine with obs_layout="split", and the first Linear -- built for the flat
row, 2 P + 14 ('raw': P + 18) input columns plus those of x2 -- reads the flat row they stand for, rebuilt from the engine's market
series while it loads (include/ptg_env.h: PTG_MLP_SPLIT_INPUT).  Outputs and gradients have the bits of the
obs="flat" call on policy_split.flat_rows_from_split(x); nothing is rebuilt after a weight update.

    policy = DeviceMLP(engine, q_net, batch=engine.n, obs="split");  logits = policy(engine.obs)

Not supported: float64 nets (a float64 engine's split rows too); a Linear without bias; anything but Linear / ReLU / Tanh in the
sequence.  There is no torch fall-back.

Cost (profiles/mlp_cost.txt; DESIGN.md section 18 has the table and its one condition, which is MISSED at 7 of its 12 shapes).  Device time
against the same nn.Sequential under torch.no_grad(): faster for the deep, narrow nets at the reference's batch sizes (DQN's 7 x 366 at B = 6
and 544: 1.6x - 1.8x; SAC's 6 x 233 critic at 6 and 470: 1.9x; PPO's 2 x 358 at 203: 1.09x), SLOWER for the wide ones there (A2C's 4 x 808 at
B = 6 and 658: 0.69x and 0.56x; TQC's 3 x 708 critic at 6 and 290: 0.64x; TD3's 3 x 743 critic at 6 and 257: 0.84x and 0.87x; PPO at B = 6:
0.85x) and slower at thousands of rows (0.47x - 1.01x of the vendor GEMM at 4 096 - 65 536).  Inside a captured collect loop with a
40 -> 64 -> 64 -> 5 policy it is faster than torch's kernels at 4 096 envs and slower at 65 536.  What it gives at every shape is the fixed summation order -- the same bits for a row at every
batch size -- and calls that capture into a graph without allocation."""
import torch

from . import _lib


def parse_mlp(modules):
    """(linears, hidden_activation, out_activation) of an nn.Sequential, a Linear, or a list of those to chain.  TypeError for a module
    that is not Linear / ReLU / Tanh / Sequential of them or a parameter that is not float32; then ValueError for a sequence that is not
    Linear (activation Linear)* [activation], for mixed hidden activations, for a Linear without bias and for too many layers."""
    nn = torch.nn
    flat = []

    def walk(m):
        if isinstance(m, nn.Sequential) or isinstance(m, (list, tuple)):
            for c in m:
                walk(c)
        elif isinstance(m, (nn.Linear, nn.ReLU, nn.Tanh)):
            flat.append(m)
        else:
            raise TypeError(f"DeviceMLP: only Linear, ReLU and Tanh (in a Sequential or a list) are supported, got {type(m).__name__}")

    walk(modules)
    for m in flat:
        if isinstance(m, nn.Linear):
            for name, p in (("weight", m.weight), ("bias", m.bias)):
                if p is not None and p.dtype != torch.float32:
                    raise TypeError(f"DeviceMLP: Linear.{name} must be torch.float32, got {p.dtype}")
    linears, acts = [], []                                   # acts[l]: the activation behind linears[l], or None
    for m in flat:
        if isinstance(m, nn.Linear):
            linears.append(m)
            acts.append(None)
        elif not linears or acts[-1] is not None:
            raise ValueError("DeviceMLP: an activation must follow a Linear, one at most")
        else:
            acts[-1] = "relu" if isinstance(m, nn.ReLU) else "tanh"
    if not 1 <= len(linears) <= _lib.MLP_MAX_LAYERS:
        raise ValueError(f"DeviceMLP: 1 to {_lib.MLP_MAX_LAYERS} Linear layers, got {len(linears)}")
    hidden = set(acts[:-1])
    if None in hidden:
        raise ValueError("DeviceMLP: two Linear layers with no activation between them")
    if len(hidden) > 1:
        raise ValueError("DeviceMLP: mixed hidden activations; one of ReLU and Tanh serves every hidden layer")
    for l, m in enumerate(linears):
        if m.bias is None:
            raise ValueError(f"DeviceMLP: Linear {l} has no bias")
        if l and m.in_features != linears[l - 1].out_features:
            raise ValueError(f"DeviceMLP: Linear {l} takes {m.in_features} features, Linear {l - 1} gives {linears[l - 1].out_features}")
    return linears, (hidden.pop() if hidden else "relu"), acts[-1]


class _NetBuffers:
    """What DeviceMLP and TrainMLP share: the parsed net, held by reference and checked to be contiguous and on the engine's device, and
    the output and the forward's workspace for `batch` rows.  The messages carry the subclass's name."""

    def __init__(self, engine, modules, batch, hidden=False, obs="flat"):
        """engine: the HipEngine whose device and library serve the calls; modules: see parse_mlp; batch: the most rows a call takes;
        hidden: keep the post-activation hidden layers of the last call in `self.hidden` (views into the workspace: what a backward
        pass would read); obs: "flat", or "split" for split observation rows as x (the module's docstring)."""
        who = type(self).__name__
        if obs not in ("flat", "split"):
            raise ValueError(f"{who}: obs must be 'flat' or 'split', got {obs!r}")
        self.split = obs == "split"
        self.engine = engine
        self.linears, self.hidden_activation, self.out_activation = parse_mlp(modules)
        for l, m in enumerate(self.linears):
            if not m.weight.is_contiguous() or not m.bias.is_contiguous():
                raise ValueError(f"{who}: the parameters of Linear {l} must be contiguous, got weight strides {tuple(m.weight.stride())}")
        for l, m in enumerate(self.linears):
            for p in (m.weight, m.bias):
                if p.device != engine.device:
                    raise ValueError(f"{who}: Linear {l} lives on {p.device}, the engine on {engine.device}")
        self.batch = int(batch)
        self.widths = [m.out_features for m in self.linears]
        self.in_features = self.linears[0].in_features
        self.keep_hidden = bool(hidden)
        nbytes = engine.mlp_workspace(self.batch, self.widths, self.keep_hidden)      # ValueError for a batch or a width out of range
        with engine._torch.cuda.device(engine.device):
            self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=engine.device)
            self.out = torch.empty((self.batch, self.widths[-1]), dtype=torch.float32, device=engine.device)
        self.hidden = None

    def _rows(self, x):
        """the rows of a [B, F] tensor, at most `batch`; None for what mlp_forward refuses itself"""
        B = x.shape[0] if torch.is_tensor(x) and x.dim() == 2 else None
        if B is not None and B > self.batch:
            raise ValueError(f"{type(self).__name__}: {B} rows, allocated for {self.batch}")
        return B

    def params(self):
        """(weights, biases) as the ops take them: the parameters where they are now, detached"""
        return [m.weight.detach() for m in self.linears], [m.bias.detach() for m in self.linears]


class DeviceMLP(_NetBuffers):
    def __call__(self, x, x2=None):
        """x [B, F1] (and x2 [B, F2]) float32 with B <= batch -> the output [B, O]: the first B rows of the preallocated tensor, which
        the next call overwrites.  Reads the parameters where they are now."""
        B = self._rows(x)
        res = self.engine.mlp_forward(x, *self.params(), hidden_activation=self.hidden_activation, out_activation=self.out_activation, x2=x2,
                                      out=None if B is None else self.out[:B], workspace=self.workspace, keep_hidden=self.keep_hidden, split=self.split)
        self.hidden = res.hidden
        return res.out


def _backward_plan(net, x, x2, grad_out, need_x, need_x2, need_params):
    """One network's share of a backward call, for both autograd functions.  net: a TrainMLP; x, x2: what its forward saved; need_x, need_x2,
    need_params (w0, b0, w1, b1, ...): its entries of needs_input_grad.  A split net has no grad_x, and its grad_input holds the x2 part alone.  Returns grad_out with rows the op accepts, grad_weights and grad_biases
    (None for a layer that needs neither; both None when no layer does), grad_x and grad_x2 (views into net.grad_input, or None) and grads, the network's entries of what backward() returns."""
    B, F1 = x.shape[0], (0 if net.split else x.shape[1])
    if grad_out.stride(1) != 1 or (B > 1 and grad_out.stride(0) < grad_out.shape[1]):
        grad_out = grad_out.contiguous()                     # e.g. the expanded gradient of a sum
    n = len(net.linears)
    wanted = [need_params[2 * l] or need_params[2 * l + 1] for l in range(n)]
    gw = [net.grad_weights[l] if wanted[l] else None for l in range(n)] if any(wanted) else None
    gb = [net.grad_biases[l] if wanted[l] else None for l in range(n)] if any(wanted) else None
    gx = net.grad_input[:B, :F1] if need_x and not net.split else None
    gx2 = net.grad_input[:B, F1:] if x2 is not None and need_x2 else None
    grads = []
    for l in range(n):
        grads += [gw[l] if gw is not None and need_params[2 * l] else None, gb[l] if gb is not None and need_params[2 * l + 1] else None]
    return grad_out, gw, gb, gx, gx2, grads


class _TrainMLPFunction(torch.autograd.Function):
    """forward: mlp_forward with keep_hidden into the module's buffers; backward: mlp_backward into the module's gradient buffers"""

    @staticmethod
    def forward(ctx, net, x, x2, *params):
        B = net._rows(x)
        xd, x2d = (x.detach() if torch.is_tensor(x) else x), (x2.detach() if torch.is_tensor(x2) else x2)
        res = net.engine.mlp_forward(xd, [p.detach() for p in params[0::2]], [p.detach() for p in params[1::2]], hidden_activation=net.hidden_activation,
                                     out_activation=net.out_activation, x2=x2d, out=None if B is None else net.out[:B], workspace=net.workspace,
                                     keep_hidden=True, split=net.split)
        net.calls += 1
        net.hidden = res.hidden
        ctx.net, ctx.call, ctx.x, ctx.x2 = net, net.calls, xd, x2d
        return res.out

    @staticmethod
    def backward(ctx, grad_out):
        net = ctx.net
        if ctx.call != net.calls:
            raise RuntimeError(f"TrainMLP: backward of forward call {ctx.call}, but the latest forward is call {net.calls}: the kept activations live in the "
                               "module's workspace and a later forward has overwritten them (run each backward before the next forward)")
        x, x2 = ctx.x, ctx.x2
        needs = ctx.needs_input_grad                         # (net, x, x2, w0, b0, w1, b1, ...)
        grad_out, gw, gb, gx, gx2, grads = _backward_plan(net, x, x2, grad_out, needs[1], needs[2], needs[3:])
        net._views = (gx, gx2)                               # held here too, so that autograd copies them into a leaf's .grad and never adopts them
        net.engine.mlp_backward(grad_out, x, *net.params(), net.out[:x.shape[0]], net.workspace, hidden_activation=net.hidden_activation,
                                out_activation=net.out_activation, x2=x2, grad_weights=gw, grad_biases=gb, grad_x=gx, grad_x2=gx2,
                                backward_workspace=net.backward_workspace, split=net.split)
        return (None, gx, gx2, *grads)


class TrainMLP(_NetBuffers):
    """The training forward and backward of a torch MLP under autograd, on the project's kernels (HipEngine.mlp_forward with keep_hidden and
    HipEngine.mlp_backward; include/ptg_env.h states both arithmetics, DESIGN.md section 19 the design).

        q_net = TrainMLP(engine, q_net_module, batch=544)
        loss_grad = ...                                                   # e.g. engine.td_loss(...).grad_q
        q = q_net(obs);  q.backward(loss_grad);  optimiser.step()         # .grad of every parameter from k_mlp_dw, of obs from k_mlp_dx
        critic = TrainMLP(engine, qf, batch=256);  critic(obs, x2=actions)   # th.cat([obs, action], 1) without the cat

    The parameters are held BY REFERENCE.  The output, the kept activations, both workspaces and the gradient buffers are allocated once,
    for `batch` rows, and every call overwrites them: the output of a call is valid until the next call, and backward() must run before the
    next forward of the same TrainMLP -- a backward whose forward is no longer the latest one raises RuntimeError (a call counter, not a
    copy).  The tensors backward() returns to autograd are the module's own gradient buffers; autograd copies them into `.grad` (or adds
    them to it), so `.grad` stays valid when the buffers are reused.  Parameters with requires_grad False launch no weight-gradient kernel
    and keep `.grad` None; an input that needs no gradient gets no first-layer input-gradient launch.
    obs="split": x is split observation rows (the module's docstring); their gradient is None, whatever x.requires_grad says, and
    grad_input holds the x2 part alone.
    Not supported: float64 nets, a Linear without bias, anything but Linear / ReLU / Tanh.  There is no torch fall-back.
    Cost (profiles/mlp_backward_cost.txt; DESIGN.md section 19 has the table and its one condition -- forward + backward not above the same
    nn.Sequential's under autograd at each agent's own batch size -- which is MISSED at 5 of its 6 shapes): torch's device time of forward +
    backward over this route's (below 1: slower than torch), TrainMLP / the two raw library calls into preallocated .grad tensors: DQN 7 x 366 at B = 544 0.75x / 0.98x, A2C
    4 x 808 at 658 0.52x / 0.58x, PPO 2 x 358 at 203 0.89x / 1.95x, TD3's 3 x 743 critic at 257 0.70x / 0.97x, TQC's 3 x 708 critic at 290
    0.69x / 0.95x; SAC's 6 x 233 critic at 470 1.55x / 2.24x; at B = 6 0.85x - 1.52x / 1.2x - 6.5x.  TrainMLP's own overhead
    over the raw calls (70 - 230 us: the autograd function, two sets of argument checks, autograd's copies into .grad) is most of the
    miss; a captured gradient step calls mlp_forward and mlp_backward directly.  What the route gives at every shape is the fixed order."""

    def __init__(self, engine, modules, batch, obs="flat"):
        super().__init__(engine, modules, batch, hidden=True, obs=obs)
        if self.split:
            from .policy_split import flat_columns
            flat = flat_columns("mod" if engine.consts["raw_modified"] else "raw", int(engine.consts["price_ahead"]))[1]
            if self.in_features < flat:
                raise ValueError(f"TrainMLP: the first Linear takes {self.in_features} features, the flat observation alone has {flat}")
        nback = engine.mlp_backward_workspace(self.batch, self.widths)
        dev = engine.device
        with engine._torch.cuda.device(dev):
            self.backward_workspace = torch.empty(nback, dtype=torch.uint8, device=dev)
            self.grad_input = torch.empty((self.batch, self.in_features - (flat if self.split else 0)), dtype=torch.float32, device=dev)
            self.grad_weights = [torch.empty_like(m.weight, requires_grad=False) for m in self.linears]
            self.grad_biases = [torch.empty_like(m.bias, requires_grad=False) for m in self.linears]
        self._views = None
        self.calls = 0

    def parameters(self):
        return [p for m in self.linears for p in (m.weight, m.bias)]

    def __call__(self, x, x2=None):
        """x [B, F1] (and x2 [B, F2]) float32 with B <= batch -> the output [B, O] with a grad_fn: the first B rows of the preallocated
        tensor, which the next call overwrites"""
        return _TrainMLPFunction.apply(self, x, x2, *self.parameters())


def _group_members(who, kind, engine, nets, batch, obs="flat"):
    """one `kind` (DeviceMLP or TrainMLP) per entry of nets, once the group is 1 to MLP_GROUP_MAX networks of equal depth and activations"""
    if not isinstance(nets, (list, tuple)):
        raise TypeError(f"{who}: nets must be a list with what DeviceMLP takes for each network, got {type(nets).__name__}")
    if not 1 <= len(nets) <= _lib.MLP_GROUP_MAX:
        raise ValueError(f"{who}: 1 to {_lib.MLP_GROUP_MAX} networks, got {len(nets)}")
    parsed = [parse_mlp(m) for m in nets]
    for i, (linears, hidden, out) in enumerate(parsed):
        if len(linears) != len(parsed[0][0]):
            raise ValueError(f"{who}: nets 0 and {i} disagree in depth: {len(parsed[0][0])} and {len(linears)} Linear layers")
        if len(linears) > 1 and hidden != parsed[0][1]:
            raise ValueError(f"{who}: nets 0 and {i} disagree in the hidden activation: {parsed[0][1]} and {hidden}")
        if out != parsed[0][2]:
            raise ValueError(f"{who}: nets 0 and {i} disagree in the output activation: {parsed[0][2]} and {out}")
    return [kind(engine, m, batch, obs=obs) for m in nets]


def _group_inputs(who, members, x, x2):
    """(xs, x2s, B) of a group call: x and x2 each one tensor for all networks or a list with one entry per network"""
    G = len(members)
    xs = list(x) if isinstance(x, (list, tuple)) else [x] * G
    x2s = list(x2) if isinstance(x2, (list, tuple)) else [x2] * G
    if len(xs) != G or len(x2s) != G:
        raise ValueError(f"{who}: {G} networks, got {len(xs)} inputs x and {len(x2s)} inputs x2")
    return xs, x2s, [m._rows(t) for m, t in zip(members, xs)]


class DeviceMLPGroup:
    """Up to 8 DeviceMLPs of equal depth and activations in ONE launch per layer (HipEngine.mlp_group_forward; include/ptg_env.h:
    ptg_mlp_group_forward): the two target critics of TD3 / SAC / TQC on (next_obs, next_action), critics and
    their targets, PPO's policy and value nets on one observation batch.  Every output is, bit for bit, what a DeviceMLP of that network
    returns.

        targets = DeviceMLPGroup(engine, [qf0_target, qf1_target], batch=256)
        q0, q1 = targets(next_obs, x2=next_actions)                       # a tensor is shared by all networks; a list gives each its own

    nets: a list of what DeviceMLP takes, one entry per network; widths and input sizes may differ, depth and activations may not
    (ValueError, which names the two networks).  DeviceMLP's rules hold: the parameters are held BY REFERENCE, output and workspace of
    every network are allocated once for `batch` rows, a call returns the first B rows of them and the next call overwrites them.
    Cost (profiles/mlp_group_cost.txt; DESIGN.md section 20 has the table and its one condition -- the grouped raw call's median not above
    the G single calls' taken in turn -- which HELD at every shape).  Device time of the forward, the G single mlp_forward calls over the
    grouped call / the same nn.Sequentials under no_grad over DeviceMLPGroup: TD3's twin critics 3 x 743 at B = 257 1.71x / 2.04x, SAC's
    6 x 233 at 470 1.57x / 2.92x, TQC's 3 x 708 at 290 1.70x / 1.79x, PPO's pi + vf 2 x 358 at 203 1.86x / 3.65x, A2C's pi + vf 4 x 808 at
    658 1.21x / 0.97x (LEVEL WITH TORCH, NOT AHEAD: the single network's grid already exceeds the chip there), SAC's two critics and two
    targets at 470 1.49x / 3.10x; at B = 6 1.66x - 1.99x / 1.93x - 3.67x.  DeviceMLPGroup costs 5 - 57 us more than the raw grouped call
    (a second set of argument checks).  A FIRST RUN of the tool, with the grouped route first in every repetition, read the grouped
    forward ABOVE the single calls for SAC's critics (144 against 114 us at B = 6, 155 against 126 at 470) and PPO's pi + vf (72 against
    48 at 6, 71 against 53 at 203) while this class read 44 and 42 us for PPO in the same run: the first place in a repetition cost
    that, not the grouped kernels; the figures above are from the run in which the first place rotates.  A grouped call makes the checks of all its networks before its first launch; on an idle stream
    that host time (70 - 180 us) is not hidden, which was not measured."""

    def __init__(self, engine, nets, batch, obs="flat"):
        """obs: "flat", or "split" for split observation rows as every network's x (the module's docstring)"""
        self.engine = engine
        self.nets = _group_members("DeviceMLPGroup", DeviceMLP, engine, nets, batch, obs)
        self.batch = int(batch)

    def __call__(self, x, x2=None):
        """x [B, F1] (and x2 [B, F2]) float32 shared by all networks, or lists with one tensor per network -> the tuple of the G outputs"""
        xs, x2s, Bs = _group_inputs("DeviceMLPGroup", self.nets, x, x2)
        m0 = self.nets[0]
        weights, biases = zip(*[net.params() for net in self.nets])
        res = self.engine.mlp_group_forward(xs, list(weights), list(biases), hidden_activation=m0.hidden_activation, out_activation=m0.out_activation, x2s=x2s,
                                            outs=[None if B is None else net.out[:B] for net, B in zip(self.nets, Bs)], workspaces=[net.workspace for net in self.nets],
                                            split=m0.split)
        return tuple(r.out for r in res)


class _TrainMLPGroupFunction(torch.autograd.Function):
    """forward: mlp_group_forward with keep_hidden into the members' buffers; backward: one mlp_group_backward over the networks whose
    output received a gradient"""

    @staticmethod
    def forward(ctx, grp, *args):                            # args: x of every network, x2 of every network, then every network's parameters
        G = len(grp.nets)
        det = lambda t: t.detach() if torch.is_tensor(t) else t
        xs, x2s, params = [det(t) for t in args[:G]], [det(t) for t in args[G:2 * G]], args[2 * G:]
        Bs = [net._rows(t) for net, t in zip(grp.nets, xs)]
        weights, biases, at = [], [], 0
        for net in grp.nets:
            n = len(net.linears)
            weights.append([p.detach() for p in params[at:at + 2 * n:2]])
            biases.append([p.detach() for p in params[at + 1:at + 2 * n:2]])
            at += 2 * n
        m0 = grp.nets[0]
        res = grp.engine.mlp_group_forward(xs, weights, biases, hidden_activation=m0.hidden_activation, out_activation=m0.out_activation, x2s=x2s,
                                           outs=[None if B is None else net.out[:B] for net, B in zip(grp.nets, Bs)],
                                           workspaces=[net.workspace for net in grp.nets], keep_hidden=True, split=m0.split)
        grp.calls += 1
        for net, r in zip(grp.nets, res):
            net.hidden = r.hidden
        ctx.grp, ctx.call, ctx.xs, ctx.x2s = grp, grp.calls, xs, x2s
        ctx.set_materialize_grads(False)                     # an unused output's gradient arrives as None, not as zeros
        return tuple(r.out for r in res)

    @staticmethod
    def backward(ctx, *grad_outs):
        grp = ctx.grp
        if ctx.call != grp.calls:
            raise RuntimeError(f"TrainMLPGroup: backward of forward call {ctx.call}, but the latest forward is call {grp.calls}: the kept activations live in the "
                               "group's workspaces and a later forward has overwritten them (run each backward before the next forward)")
        G = len(grp.nets)
        needs = ctx.needs_input_grad                         # (grp, x_0 .. x_G-1, x2_0 .. x2_G-1, w, b, w, b, ... network by network)
        gxs, gx2s, grads = [None] * G, [None] * G, []
        rows = []                                            # per network that takes part: its arguments in mlp_group_backward's order
        at = 1 + 2 * G
        for i, net in enumerate(grp.nets):
            n = len(net.linears)
            mine = needs[at:at + 2 * n]
            at += 2 * n
            if grad_outs[i] is None:                         # this network's output was not used: it is left out of the call
                grads += [None] * (2 * n)
                continue
            x, x2 = ctx.xs[i], ctx.x2s[i]
            g, gw, gb, gxs[i], gx2s[i], own = _backward_plan(net, x, x2, grad_outs[i], needs[1 + i], needs[1 + G + i], mine)
            grads += own
            rows.append((g, x, *net.params(), net.out[:x.shape[0]], net.workspace, x2, gw, gb, gxs[i], gx2s[i], net.backward_workspace))
        grp._views = (gxs, gx2s)                             # held here too, so that autograd copies them into a leaf's .grad and never adopts them
        if rows:
            m0 = grp.nets[0]
            g, xs, weights, biases, outs, works, x2s, gws, gbs, dxs, dx2s, bws = (list(col) for col in zip(*rows))
            grp.engine.mlp_group_backward(g, xs, weights, biases, outs, works, hidden_activation=m0.hidden_activation, out_activation=m0.out_activation, x2s=x2s,
                                          grad_weights=gws, grad_biases=gbs, grad_xs=dxs, grad_x2s=dx2s, backward_workspaces=bws, split=m0.split)
        return (None, *gxs, *gx2s, *grads)


class TrainMLPGroup:
    """Up to 8 TrainMLPs of equal depth and activations under ONE autograd function with G outputs: the forward is one launch per layer
    (HipEngine.mlp_group_forward with keep_hidden), the backward one mlp_group_backward -- the launches of a single network's backward --
    over the networks whose output received a gradient (include/ptg_env.h: ptg_mlp_group_backward).  Every output
    and every gradient is, bit for bit, what a TrainMLP of that network gives.

        critics = TrainMLPGroup(engine, [qf0, qf1], batch=256)
        q0, q1 = critics(obs, x2=actions)                                 # a tensor is shared by all networks; a list gives each its own
        torch.autograd.backward([q0, q1], [grad_q0, grad_q1])            # ONE backward over both: .grad of every parameter of both critics

    A network whose output received no gradient is left out of the backward call and its parameters keep `.grad` as it was; a network
    whose parameters all have requires_grad False launches no weight-gradient work; an input without requires_grad gets no first-layer
    input gradient.  Both outputs must go into ONE backward pass (torch.autograd.backward on a list, or a loss that uses all of them):
    q0.backward() followed by q1.backward() is two passes through the function, two grouped calls.
    AN INPUT SHARED BY SEVERAL NETWORKS is handed to the function once per network, so its `.grad` is AUTOGRAD'S OWN SUM of the networks'
    input gradients, added in network order in float32; nothing is summed inside a kernel, and each network's dx is the single op's.
    TrainMLP's rules hold: parameters BY REFERENCE; every buffer allocated once for `batch` rows and overwritten by every call; backward()
    before the next forward of the same group, else RuntimeError; the gradient buffers are copied into `.grad` by autograd, never adopted.
    parameters(): all networks' parameters in network order.
    Cost (profiles/mlp_group_cost.txt; DESIGN.md section 20 has the table and its one condition -- the grouped raw calls' median not above
    the G single calls' taken in turn -- which HELD at every shape).  Device time of forward + backward, the G single raw calls over the
    grouped raw calls / the same nn.Sequentials under autograd over TrainMLPGroup (below 1: slower than torch): TD3's twin critics 3 x 743
    at B = 257 1.29x / 0.98x, SAC's 6 x 233 at 470 1.51x / 2.26x, TQC's 3 x 708 at 290 1.48x / 1.04x, PPO's pi + vf 2 x 358 at 203
    1.15x / 1.39x, A2C's pi + vf 4 x 808 at 658 1.07x / 0.58x (SLOWER THAN TORCH: 1556 against 906 us; the grouped raw calls are 0.65x
    there, the wide-net loss of TrainMLP, which a group does not cure); at B = 6 1.05x - 1.56x / 1.22x - 1.81x.  TrainMLPGroup costs
    110 - 290 us more than the raw grouped calls (the autograd function, a second set of argument checks, autograd's copies into
    .grad); a captured gradient step calls mlp_group_forward and mlp_group_backward directly."""

    def __init__(self, engine, nets, batch, obs="flat"):
        """obs: "flat", or "split" for split observation rows as every network's x (TrainMLP's rules: no gradient of x)"""
        self.engine = engine
        self.nets = _group_members("TrainMLPGroup", TrainMLP, engine, nets, batch, obs)
        self.batch = int(batch)
        self._views = None
        self.calls = 0

    def parameters(self):
        return [p for net in self.nets for p in net.parameters()]

    def __call__(self, x, x2=None):
        """x [B, F1] (and x2 [B, F2]) float32 shared by all networks, or lists with one tensor per network -> the tuple of the G outputs,
        each with a grad_fn"""
        xs, x2s, _ = _group_inputs("TrainMLPGroup", self.nets, x, x2)
        return _TrainMLPGroupFunction.apply(self, *xs, *x2s, *self.parameters())
