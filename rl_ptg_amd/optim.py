"""DeviceOptimizer: clip_grad_norm_ + torch.optim.Adam / RMSprop + SB3's polyak_update + zero_grad as ONE library call per step
(HipEngine.optim_step, include/ptg_env.h: ptg_optim_step, which states the arithmetic).

    opt = DeviceOptimizer(engine, net.parameters(), kind="adam", lr=3e-4, eps=1e-5, max_grad_norm=0.5, zero_grad=True)
    loss, stats = ppo_loss(engine, ...)
    loss.backward()
    opt.step()                                                # three launches whatever the number of tensors; no synchronisation

Differences from torch.optim, all stated in the header: every parameter of the optimiser must have a gradient when step() runs (torch
skips a parameter whose .grad is None; here that raises ValueError); the gradients are not rewritten by the clipping; all tensors share
one dtype, float32 or float64, and are contiguous; no weight decay, amsgrad, momentum or centering.  There is no torch fall-back."""
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
