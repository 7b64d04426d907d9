"""DeviceOptimizer: clip_grad_norm_ + torch.optim.Adam / RMSprop + SB3's polyak_update + zero_grad as ONE library call per step
(HipEngine.optim_step, include/ptg_env.h: ptg_optim_step, which states the arithmetic).

    opt = DeviceOptimizer(engine, net.parameters(), kind="adam", lr=3e-4, eps=1e-5, max_grad_norm=0.5, zero_grad=True)
    loss, stats = ppo_loss(engine, ...)
    loss.backward()
    opt.step()                                                # three launches whatever the number of tensors; no synchronisation

Differences from torch.optim, all stated in the header: every parameter of the optimiser must have a gradient when step() runs (torch
skips a parameter whose .grad is None; here that raises ValueError); the gradients are not rewritten by the clipping; all tensors share
one dtype, float32 or float64, and are contiguous; no weight decay, amsgrad, momentum or centering.  There is no torch fall-back.

DeviceOptimizerGroup: the steps of up to eight DeviceOptimizers -- independent agents -- as ONE library call (HipEngine.optim_step_group,
ptg_optim_step_group)."""
import torch

from .train_ops import OptimPlan  # noqa: F401  (re-exported: what DeviceOptimizer.plan is)


class DeviceOptimizer:
    def __init__(self, engine, params, kind="adam", lr=1e-3, betas=(0.9, 0.999), eps=None, alpha=0.99, max_grad_norm=None, targets=None, tau=None,
                 zero_grad=False):
        """params: the parameters (leaf tensors; their .grad is read at step()); kind "adam" | "rmsprop"; lr a float or a float64
        device tensor of 1 element (read on the device at every step: anneal it in place); eps None: torch's default, 1e-8 for both
        kinds (SB3 passes 1e-5); max_grad_norm None: no clipping and no norm pass; targets with tau: the target networks' parameters,
        moved by SB3's polyak_update after every step; zero_grad: the step leaves every gradient zeroed (set_to_none=False)."""
        if kind not in ("adam", "rmsprop"):
            raise ValueError(f"DeviceOptimizer: kind must be 'adam' or 'rmsprop', got {kind!r}")
        self.engine, self.kind = engine, kind
        self.params = list(params)
        self.targets = None if targets is None else list(targets)
        if not self.params:
            raise ValueError("DeviceOptimizer: an empty parameter list")
        if (self.targets is None) != (tau is None):
            raise ValueError("DeviceOptimizer: targets and tau go together")
        if tau is not None and not 0.0 <= float(tau) <= 1.0:
            raise ValueError(f"DeviceOptimizer: tau must be in [0, 1], got {tau}")
        if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:
            raise ValueError(f"DeviceOptimizer: max_grad_norm must be >= 0 (or None), got {max_grad_norm}")
        if torch.is_tensor(lr) and (lr.dtype != torch.float64 or lr.numel() != 1):
            raise TypeError(f"DeviceOptimizer: a tensor lr must be float64 with 1 element, got {lr.dtype} {tuple(lr.shape)}")
        self.lr, self.betas, self.eps, self.alpha = lr, (float(betas[0]), float(betas[1])), 1e-8 if eps is None else float(eps), float(alpha)
        self.max_grad_norm, self.tau, self.zero_grad_flag = max_grad_norm, tau, bool(zero_grad)
        self.plan, self._retired = None, None

    # ------------------------------------------------------------------ the step
    def _grads(self):
        return [p.grad for p in self.params]

    def _detached(self, xs):
        return None if xs is None else [x.detach() for x in xs]

    def _build(self, state=None):
        grads = self._grads()
        for k, g in enumerate(grads):
            if g is None:
                raise ValueError(f"DeviceOptimizer: parameter {k} has no gradient (torch.optim skips such a parameter; here every parameter takes the step)")
        self.plan = self.engine.optim_plan(self._detached(self.params), grads, self.kind, targets=self._detached(self.targets), state=state)

    def step(self):
        """One step of every parameter on the current stream; returns nothing.  The .grad pointers are compared with the plan's on the
        host: if one moved (zero_grad(set_to_none=True), a fresh backward) the tables are rebuilt -- under stream capture that raises.
        The plan that a rebuild replaces is kept until the following rebuild, so a step still in flight keeps its tables; beyond that, as
        with every tensor torch hands out, steps of one optimizer belong on one stream (or behind an explicit wait)."""
        grads = self._grads()
        if self.plan is None or [None if g is None else g.data_ptr() for g in grads] != self.plan.grad_ptrs:
            if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("DeviceOptimizer.step: a .grad moved (or no step was taken yet) -- the tables cannot be rebuilt under stream capture; "
                                   "take one eager step first and keep the gradients in place (zero_grad=True here, or set_to_none=False)")
            self._retired = self.plan                       # its tables, scratch and gradients stay alive until the next rebuild: a step
            self._build(state=self.plan)                    # enqueued on another stream may still be reading them
        self.engine.optim_step(self.plan, self.lr, betas=self.betas, eps=self.eps, alpha=self.alpha, max_grad_norm=self.max_grad_norm, tau=self.tau,
                               zero_grad=self.zero_grad_flag)

    def zero_grad(self, set_to_none=False):
        """torch's zero_grad; set_to_none=False by default here, so that the gradient pointers stay where the tables have them"""
        for p in self.params:
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.zero_()

    @property
    def grad_norm(self):
        """the float64 device scalar [1] with the total norm of the last step (what clip_grad_norm_ returns); None without clipping
        or before the first step"""
        return None if self.plan is None or self.max_grad_norm is None else self.plan.norm

    # ------------------------------------------------------------------ checkpoints in torch.optim's layout
    def _names(self):
        return ("exp_avg", "exp_avg_sq") if self.kind == "adam" else ("square_avg",)

    def state_dict(self):
        """torch.optim's layout: {"state": {k: {"step", "exp_avg", "exp_avg_sq"} (RMSprop: {"step", "square_avg"})}, "param_groups":
        [...]}; a checkpoint moves between this and torch's optimizer.  Synchronises (the step count is read from the device)."""
        state = {}
        if self.plan is not None:
            step = float(self.plan.state[0])
            for k in range(len(self.params)):
                st = {"step": torch.tensor(step, dtype=torch.float32)}
                for name, xs in zip(self._names(), (self.plan.state1, self.plan.state2)):
                    st[name] = xs[k].clone()
                state[k] = st
        group = {"lr": float(self.lr), "eps": self.eps, "params": list(range(len(self.params)))}
        group.update({"betas": self.betas} if self.kind == "adam" else {"alpha": self.alpha})
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd):
        """Takes a state_dict of this class or of torch.optim.Adam / RMSprop over the same parameters in the same order: the moments are
        copied, the step count t (one for all parameters) sets the device state {t, beta1^t, beta2^t}.  lr, eps, betas and alpha of its
        param group are taken over when present (a tensor lr of this optimizer is written in place)."""
        groups = sd.get("param_groups") or [{}]
        if len(groups) != 1:
            raise ValueError("DeviceOptimizer.load_state_dict: one param group expected")
        order = list(groups[0].get("params", range(len(self.params))))
        if len(order) != len(self.params):
            raise ValueError(f"DeviceOptimizer.load_state_dict: {len(self.params)} parameters here, {len(order)} in the state_dict")
        state = sd.get("state", {})
        if state and sorted(state.keys()) != sorted(order):
            raise ValueError("DeviceOptimizer.load_state_dict: every parameter or none must have state")
        steps = {float(state[k]["step"]) for k in order} if state else set()
        if len(steps) > 1:
            raise ValueError(f"DeviceOptimizer.load_state_dict: the parameters have different step counts {sorted(steps)}; here one count serves all")
        for k in order if state else ():
            for name, p in zip(self._names(), (self.params[order.index(k)],) * 2):
                if name not in state[k] or tuple(state[k][name].shape) != tuple(p.shape):
                    raise ValueError(f"DeviceOptimizer.load_state_dict: state of parameter {k} lacks {name} of shape {tuple(p.shape)}")
        g = groups[0]
        if "lr" in g:
            if torch.is_tensor(self.lr):
                self.lr.fill_(float(g["lr"]))
            else:
                self.lr = float(g["lr"])
        self.eps = float(g.get("eps", self.eps))
        if self.kind == "adam" and "betas" in g:
            self.betas = (float(g["betas"][0]), float(g["betas"][1]))
        if self.kind == "rmsprop" and "alpha" in g:
            self.alpha = float(g["alpha"])
        if not state:
            self.plan = None
            return
        if self.plan is None:
            for p in self.params:                            # a plan needs gradients in place: zeroed ones until the first backward
                if p.grad is None:
                    p.grad = torch.zeros_like(p, memory_format=torch.contiguous_format)
            self._build()
        t = steps.pop()
        for i, k in enumerate(order):
            for name, xs in zip(self._names(), (self.plan.state1, self.plan.state2)):
                xs[i].copy_(state[k][name])
        b1, b2 = self.betas if self.kind == "adam" else (1.0, 1.0)
        self.plan.state.copy_(torch.tensor([t, b1 ** t, b2 ** t, 0.0], dtype=torch.float64))


class DeviceOptimizerGroup:
    """Up to 8 DeviceOptimizers of one kind and flag set -- the optimisers of independent agents: seeds, a sweep over lr -- whose step()
    is ONE grouped library call (HipEngine.optim_step_group; include/ptg_env.h: ptg_optim_step_group): three
    launches, two without clipping, whatever the number of agents.  Every member's parameters, moments, targets, zeroed gradients, step
    count and grad norm after a step are, bit for bit, what its own DeviceOptimizer.step() gives.

        opts = [DeviceOptimizer(engine, agent.parameters(), lr=lr_i, eps=1e-5, max_grad_norm=0.5, zero_grad=True) for agent, lr_i in ...]
        group = DeviceOptimizerGroup(engine, opts)
        losses, stats = ppo_loss_group(engine, members, clip_range=0.2)
        torch.autograd.backward(losses)
        group.step()                                          # every agent's clip + Adam + zero_grad

    The members must agree in kind, in clipping or not (max_grad_norm None or not), in having targets or not and in zero_grad, and all
    parameters of all members in dtype (ValueError, which names the two members); lr (a float or a device tensor, per member), betas,
    eps, alpha, max_grad_norm and tau are each member's own, read from it at every step.  A member stays usable alone (its own step()
    takes the same next step), and checkpoints stay the members' own state_dict / load_state_dict.  As in DeviceOptimizer.step, a .grad
    that moved in a member rebuilds that member's plan; under stream capture that raises, with the member named.
    Cost (profiles/train_group_cost.txt; DESIGN.md section 26 has the table and its one condition -- at every shape the grouped route's
    median not above the G single calls', or the G single-agent graphs', taken in turn -- which HELD at every shape).  The G single calls
    over the grouped call, raw calls, HIP events behind a device-side delay: optim_step over PPO's 0.29 M parameters per member (Adam, clip,
    zero-grad) G = 2 / 4 / 6 / 8 1.54x / 2.54x / 3.43x / 3.71x (25.9 against 96.1 us at eight members), over A2C's 4 x 808 nets (RMSprop,
    clip) G = 2 / 6 1.27x / 1.64x; policy_loss at PPO's B = 203 G = 2 / 4 / 6 / 8 1.66x / 1.41x / 1.38x / 1.34x and at A2C's B = 3 948
    G = 2 / 6 1.76x / 1.87x -- from G = 4 on those loss figures hold the device waiting for the host's argument checks (in
    both routes), not one launch's device time.  A whole captured gradient step of four PPO agents (per-agent next_batch, one
    TrainMLPGroup of eight nets, ppo_loss_group, one backward, this class): 371 us per step of all four against 755 us for the four
    single-agent graphs replayed in turn, 2.03x; the four graphs on four streams read 876 us, the four gathers 9 % of the grouped replay.
    One run in one process.  Not measured: float64, the Gaussian head, G processes, the host cost of the grouped calls on an idle stream."""

    def __init__(self, engine, optimizers):
        optimizers = list(optimizers)
        if not optimizers:
            raise ValueError("DeviceOptimizerGroup: an empty list of optimizers")
        if len(optimizers) > 8:
            raise ValueError(f"DeviceOptimizerGroup: 1 to 8 optimizers, got {len(optimizers)}")
        for i, o in enumerate(optimizers):
            if not isinstance(o, DeviceOptimizer):
                raise TypeError(f"DeviceOptimizerGroup: optimizers[{i}] must be a DeviceOptimizer, got {type(o).__name__}")
        o0 = optimizers[0]
        for i, o in enumerate(optimizers):
            for name, a, b in (("kind", o0.kind, o.kind), ("clipping (max_grad_norm None or not)", o0.max_grad_norm is not None, o.max_grad_norm is not None),
                               ("having targets", o0.targets is not None, o.targets is not None), ("zero_grad", o0.zero_grad_flag, o.zero_grad_flag),
                               ("the parameters' dtype", o0.params[0].dtype, o.params[0].dtype)):
                if a != b:
                    raise ValueError(f"DeviceOptimizerGroup: optimizers 0 and {i} disagree in {name}: {a} and {b}")
            if o.engine is not engine:
                raise ValueError(f"DeviceOptimizerGroup: optimizers[{i}] belongs to another engine")
        if len({id(o) for o in optimizers}) != len(optimizers):
            raise ValueError("DeviceOptimizerGroup: an optimizer is given twice")
        self.engine, self.optimizers = engine, optimizers

    def step(self):
        """One step of every parameter of every member on the current stream; returns nothing.  Each member's .grad pointers are compared
        with its plan's, as DeviceOptimizer.step does: a member whose .grad moved has its plan rebuilt (its moments and step count are
        taken over) -- under stream capture that raises, with the member named."""
        for i, o in enumerate(self.optimizers):
            grads = o._grads()
            if o.plan is None or [None if g is None else g.data_ptr() for g in grads] != o.plan.grad_ptrs:
                if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
                    raise RuntimeError(f"DeviceOptimizerGroup.step: member {i}: a .grad moved (or no step was taken yet) -- the tables cannot be rebuilt under "
                                       "stream capture; take one eager step first and keep the gradients in place (zero_grad=True, or set_to_none=False)")
                o._retired = o.plan
                o._build(state=o.plan)
        os_ = self.optimizers
        self.engine.optim_step_group([o.plan for o in os_], [o.lr for o in os_], betas=[o.betas for o in os_], eps=[o.eps for o in os_],
                                     alpha=[o.alpha for o in os_], max_grad_norm=[o.max_grad_norm for o in os_], tau=[o.tau for o in os_],
                                     zero_grad=os_[0].zero_grad_flag)

    def zero_grad(self, set_to_none=False):
        for o in self.optimizers:
            o.zero_grad(set_to_none=set_to_none)

    @property
    def grad_norms(self):
        """the members' grad_norm: a list of float64 device scalars [1] (None without clipping or before the first step)"""
        return [o.grad_norm for o in self.optimizers]
