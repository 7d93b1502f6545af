"""``Adam`` with torch.optim.Adam's constructor, state layout and update (the optimiser of the reference's train.py:99-100), whose step
is ONE launch of the multi-tensor HIP kernel ``mi_adam_step`` (csrc/optim.hip) for all parameters on the GPU.

State per parameter: ``step`` (a host float tensor like torch's default), ``exp_avg``, ``exp_avg_sq`` -- a ``state_dict()`` of either
optimiser loads into the other.  Parameters that are not fp32 / not on the GPU / not contiguous take torch's own update.

``EMA`` keeps an exponential moving average of the parameters: one fp32 shadow per parameter, updated by ``mi_ema_update`` -- or,
attached to an ``Adam``, inside that optimiser's launch (``mi_adam_ema_step``) -- and exchanged with the live weights by ``mi_ema_swap`` for
validation and sampling (``average_parameters()``).

``clip_grad_norm_`` is torch.nn.utils.clip_grad_norm_ for the 2-norm on the device: ``mi_grad_sumsq`` -> ``mi_grad_clip_coef`` ->
``mi_grad_scale``, the norm accumulated in fp64, no host synchronisation.  ``Adam(max_grad_norm=...)`` is the deferred form: no scaling pass,
the Adam launch reads the coefficient through ``grad_scale`` and the gradients are never rewritten."""
from __future__ import annotations

import ctypes as C
from contextlib import contextmanager

import numpy as np
import torch

from . import _lib as L

CHUNK = 4096           # elements per launched workgroup

_clip_tables = {}      # clip_grad_norm_: rows -> uploaded table (bounded: cleared when full)
_partials_buf = {}     # device -> fp64 buffer of per-chunk sums of squares, grown on demand


def _partials(dev, n: int):
    buf = _partials_buf.get(dev)
    if buf is None or buf.numel() < n:
        buf = _partials_buf[dev] = torch.empty(max(n, 1024), dtype=torch.float64, device=dev)
    return buf


def _grad_block(tb, grad_scale=None) -> "L.MiAdamParams":
    """mi_adam_params over an uploaded (tensor table, chunk tensor, chunk offset, chunk count): what the mi_grad_* entries read"""
    a = L.MiAdamParams()
    a.tensors, a.chunk_tensor, a.chunk_off, a.nchunks, a.chunk = tb[0].data_ptr(), tb[1].data_ptr(), tb[2].data_ptr(), tb[3], CHUNK
    a.grad_scale = grad_scale
    return a


def _squares(g):
    """sum of squares of a gradient the kernels do not take, as a 0-dim double on its own device"""
    x = g.coalesce().values() if g.is_sparse else g
    return x.detach().to(torch.float64).pow(2).sum()


def _grad_eligible(g) -> bool:
    return g.layout == torch.strided and g.dtype == torch.float32 and g.is_contiguous() and g.numel() > 0 and (g.is_cuda or L.backend() == "hipemu")


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """torch.nn.utils.clip_grad_norm_ with the 2-norm taken and applied by three launches for all eligible gradients (dense, fp32,
    contiguous, on the GPU): ``mi_grad_sumsq`` (per-chunk sums of squares in fp64), ``mi_grad_clip_coef`` (the norm and torch's coefficient
    ``min(1, max_norm / (norm + 1e-6))``) and ``mi_grad_scale`` (in place; exits without touching memory when nothing is clipped).  The
    other gradients enter the same norm through double torch ops and are scaled by the same coefficient.  Returns the total norm before
    clipping, a 0-dim fp32 tensor on the gradients' device (a fresh one per call); the host is not synchronised unless
    ``error_if_nonfinite`` is set, which reads the norm and raises torch's ``RuntimeError`` before anything is scaled.

    The whole call is handed to ``torch.nn.utils.clip_grad_norm_`` when ``norm_type != 2``, when the eligible gradients sit on more than
    one device, and when no gradient is eligible.  No gradients at all returns ``torch.tensor(0.)`` like torch."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    parameters = list(parameters)
    max_norm, norm_type = float(max_norm), float(norm_type)
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.tensor(0.)
    fast = [g for g in grads if _grad_eligible(g)]
    if norm_type != 2.0 or not fast or len({g.device for g in fast}) > 1:
        return torch.nn.utils.clip_grad_norm_(parameters, max_norm, norm_type, error_if_nonfinite, foreach)
    if not max_norm >= 0.0:
        raise ValueError(f"clip_grad_norm_: max_norm must not be negative or NaN, got {max_norm}")
    taken = {id(g) for g in fast}
    slow = [g for g in grads if id(g) not in taken]
    dev, lib, stream = fast[0].device, L.lib(), L.current_stream()
    # (zero_grad(set_to_none=True) re-allocates the gradients: the caching allocator usually hands the same blocks back, and the table holds)
    rows = tuple((0, g.data_ptr(), 0, 0, g.numel()) for g in fast)
    tb = _clip_tables.get((dev, rows))
    if tb is None:
        if len(_clip_tables) >= 8:
            _clip_tables.clear()
        tb = _clip_tables[(dev, rows)] = _upload(rows, dev)
    partials = _partials(dev, tb[3])
    L.check(lib.mi_grad_sumsq(C.byref(_grad_block(tb)), partials.data_ptr(), stream), "mi_grad_sumsq")
    extra = None
    if slow:
        extra = torch.zeros((), dtype=torch.float64, device=dev)
        for g in slow:
            extra += _squares(g).to(dev)
    out = torch.empty(2, dtype=torch.float32, device=dev)       # fresh per call: a norm the caller keeps for logging is never overwritten
    L.check(lib.mi_grad_clip_coef(partials.data_ptr(), tb[3], extra.data_ptr() if extra is not None else None, max_norm, out.data_ptr(), stream),
            "mi_grad_clip_coef")
    if error_if_nonfinite and not bool(torch.isfinite(out[0])):
        raise RuntimeError(f"The total norm of order {norm_type} for gradients from `parameters` is non-finite, so it cannot be clipped. To disable "
                           "this error and scale the gradients by the non-finite norm anyway, set `error_if_nonfinite=False`")
    L.check(lib.mi_grad_scale(C.byref(_grad_block(tb, out.data_ptr() + 4)), stream), "mi_grad_scale")
    for g in fast:                                          # written through raw pointers: tell autograd / every version-keyed cache
        torch.autograd.graph.increment_version(g)
    for g in slow:
        g.mul_(out[1].to(g.device))
    return out[0]


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0., amsgrad: bool = False,
                 maximize: bool = False, capturable: bool = False, *, max_grad_norm=None):
        """``max_grad_norm`` (keyword-only, not in torch): clip the global 2-norm of the gradients of ALL groups at this value inside
        ``step()`` -- ``mi_grad_sumsq`` per launch table, one ``mi_grad_clip_coef``, and the Adam launches read the coefficient through
        ``grad_scale``.  The gradients themselves are NOT modified (the one visible difference from clipping in place with
        ``clip_grad_norm_``); ``optimizer.grad_norm`` is the norm before clipping of the last step, a fresh 0-dim device tensor per step
        (None before the first).  An attribute of the optimiser, not part of ``param_groups`` / ``state_dict()``.  None: exactly the
        launches of an optimiser without it."""
        if amsgrad or maximize or capturable:
            raise NotImplementedError("minimagen_amd.optim.Adam implements torch.optim.Adam's default update only (no amsgrad / maximize / capturable)")
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0 or not 0.0 <= weight_decay:
            raise ValueError("invalid Adam hyper-parameters")
        if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:
            raise ValueError(f"invalid max_grad_norm: {max_grad_norm}")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._tables = {}
        self._count = {}          # parameter -> step count as a Python int (mirrored into the state's host ``step`` tensor at every step)
        self._ema = None          # an EMA whose shadow update rides in this optimiser's launch (EMA.attach)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.grad_norm = None     # with max_grad_norm: the last step's total gradient norm before clipping (0-dim device tensor)

    def _state_of(self, p):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            self._count[p] = 0
        elif p not in self._count:                      # state that came in through load_state_dict
            self._count[p] = int(float(st["step"]))
        return st

    def state_dict(self):
        for p, n in self._count.items():
            if p in self.state:
                self.state[p]["step"].fill_(float(n))
        return super().state_dict()

    def load_state_dict(self, state_dict):
        for g in state_dict.get("param_groups", ()):
            if g.get("amsgrad") or g.get("maximize") or g.get("capturable"):
                raise NotImplementedError("minimagen_amd.optim.Adam: a state dict with amsgrad / maximize / capturable set would be silently ignored")
        super().load_state_dict(state_dict)
        self._count = {}
        self._tables = {}

    def _table(self, gi, ps):
        """device-resident tensor / chunk tables of one parameter group, rebuilt only when a pointer changed (zero_grad(set_to_none=True)
        re-allocates the gradients: the caching allocator usually hands the same blocks back)"""
        rows = [(p.data_ptr(), p.grad.data_ptr(), self.state[p]["exp_avg"].data_ptr(), self.state[p]["exp_avg_sq"].data_ptr(), p.numel()) for p in ps]
        key = tuple(rows)
        tb = self._tables.get(gi)
        if tb is not None and tb[0] == key:
            return tb
        dev = ps[0].device
        tens = np.zeros((len(rows), 5), dtype=np.int64)
        tens[:] = rows
        ct, co = [], []
        for k, r in enumerate(rows):
            n = -(-r[4] // CHUNK)
            ct += [k] * n
            co += list(range(n))
        # through pinned memory, asynchronously: zero_grad(set_to_none=True) re-allocates the gradients, so this table is rebuilt on most steps, and a
        # pageable host -> device copy waits for everything queued before it -- one full host / GPU synchronisation per training step
        up = (lambda a: torch.from_numpy(a).pin_memory().to(dev, non_blocking=True)) if dev.type == "cuda" else (lambda a: torch.from_numpy(a).to(dev))
        tb = (key, up(tens.view(np.uint8).reshape(-1)), up(np.asarray(ct, dtype=np.int32)), up(np.asarray(co, dtype=np.int32)), len(ct))
        self._tables[gi] = tb
        return tb

    def _clip_coef(self, work):
        """the deferred clip: the global 2-norm over every gradient this step takes (all groups, kernel and slow path) -> ``grad_norm``;
        returns the clip coefficient as a 0-dim fp32 tensor, on the device of the kernel-path gradients"""
        tables = [(ps, tb) for _, tabs, _ in work for _, _, ps, tb in tabs]
        slow = [p.grad for _, _, sl in work for p in sl]
        if not tables:                                      # nothing the kernels take: torch ops, the same formulas in double
            if not slow:
                self.grad_norm = torch.tensor(0.)
                return None
            S = torch.stack([_squares(g).to(slow[0].device) for g in slow]).sum()
            norm = S.sqrt()
            self.grad_norm = norm.float()
            return (self.max_grad_norm / (norm + 1e-6)).clamp(max=1.0).float()
        dev = tables[0][0][0].device
        if any(ps[0].device != dev for ps, _ in tables):
            raise NotImplementedError("minimagen_amd.optim.Adam: max_grad_norm needs the kernel-path parameters on one device")
        lib, stream = L.lib(), L.current_stream()
        n = sum(tb[4] for _, tb in tables)
        partials = _partials(dev, n)
        at = 0
        for _, tb in tables:                                # one launch per table, each into its own slice
            L.check(lib.mi_grad_sumsq(C.byref(_grad_block(tb[1:])), partials.data_ptr() + 8 * at, stream), "mi_grad_sumsq")
            at += tb[4]
        extra = None
        if slow:
            extra = torch.zeros((), dtype=torch.float64, device=dev)
            for g in slow:
                extra += _squares(g).to(dev)
        out = torch.empty(2, dtype=torch.float32, device=dev)
        L.check(lib.mi_grad_clip_coef(partials.data_ptr(), n, extra.data_ptr() if extra is not None else None, self.max_grad_norm, out.data_ptr(),
                                      stream), "mi_grad_clip_coef")
        self.grad_norm = out[0]
        return out[1]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = L.lib()
        ema = self._ema
        ema_w = ema.advance() if ema is not None else None        # None: no shadow update is due at this step -> exactly the launches of an optimiser with nothing attached
        fused = []
        work = []                                           # per group: (group, [(slot, step count, parameters, table)], slow-path parameters)
        for gi, group in enumerate(self.param_groups):
            fast, slow = [], []
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("Adam does not support sparse gradients")
                ok = p.dtype == torch.float32 and p.grad.dtype == torch.float32 and p.is_contiguous() and p.grad.is_contiguous() \
                    and (p.is_cuda or L.backend() == "hipemu") and p.device == p.grad.device
                (fast if ok else slow).append(p)
            for p in fast + slow:
                st = self._state_of(p)
                self._count[p] += 1
                st["step"].fill_(float(self._count[p]))          # a host scalar: readers of optimizer.state[p]['step'] see the live count
            # parameters of one group share the step count in every ordinary use; groups whose counts differ are split by count
            by_step = {}
            for p in fast:
                by_step.setdefault(float(self._count[p]), []).append(p)
            # (table slots are keyed by group and position among the distinct counts, not by the count itself: nothing accumulates per step)
            work.append((group, [(slot, t, ps, self._table((gi, slot), ps)) for slot, (t, ps) in enumerate(by_step.items())], slow))
        coef = self._clip_coef(work) if self.max_grad_norm is not None else None
        for gi, (group, tables, slow) in enumerate(work):
            b1, b2 = group["betas"]
            for slot, t, ps, (_, tens, ct, co, nchunks) in tables:
                a = L.MiAdamParams()
                a.tensors, a.chunk_tensor, a.chunk_off, a.nchunks, a.chunk = tens.data_ptr(), ct.data_ptr(), co.data_ptr(), nchunks, CHUNK
                a.lr, a.beta1, a.beta2, a.eps, a.weight_decay = group["lr"], b1, b2, group["eps"], group["weight_decay"]
                a.bias_correction1, a.bias_correction2 = 1.0 - b1 ** t, 1.0 - b2 ** t
                a.one_minus_beta1, a.one_minus_beta2 = 1.0 - b1, 1.0 - b2
                if coef is not None:
                    a.grad_scale = coef.data_ptr()          # (on this table's device: _clip_coef checked; kept alive by grad_norm's storage)
                rows = [ema._shadow_of.get(p) for p in ps] if ema_w is not None else None
                if rows is not None and all(e is not None and e.device == p.device for e, p in zip(rows, ps)):
                    e = ema._params(("adam", gi, slot), ps, ema_w)
                    L.check(lib.mi_adam_ema_step(C.byref(a), C.byref(e), L.current_stream()), "mi_adam_ema_step")
                    fused += ps
                else:
                    L.check(lib.mi_adam_step(C.byref(a), L.current_stream()), "mi_adam_step")
                for p in ps:                                # the kernel wrote through raw pointers: tell autograd / every version-keyed cache
                    torch.autograd.graph.increment_version(p)
            for p in slow:                                  # torch's single-tensor update, same formulas
                st = self.state[p]
                g = p.grad if coef is None else p.grad * coef.to(p.grad.device)
                g = g if group["weight_decay"] == 0 else g.add(p, alpha=group["weight_decay"])
                t = float(self._count[p])
                st["exp_avg"].lerp_(g, 1 - b1)
                st["exp_avg_sq"].mul_(b2).addcmul_(g, g, value=1 - b2)
                denom = (st["exp_avg_sq"].sqrt() / (1 - b2 ** t) ** 0.5).add_(group["eps"])
                p.addcdiv_(st["exp_avg"], denom, value=-group["lr"] / (1 - b1 ** t))
        if ema_w is not None:                               # parameters without a gradient at this step, on the slow path, or not this optimiser's
            ema._apply(ema_w, skip=fused)
        return loss


def _eligible(p, e) -> bool:
    """a (parameter, shadow) pair the kernels take: fp32, contiguous, where the loaded backend computes"""
    return p.dtype == torch.float32 and p.is_contiguous() and e.is_contiguous() and p.device == e.device and (p.is_cuda or L.backend() == "hipemu")


def _upload(rows, dev):
    """device-resident (tensor table, chunk tensor, chunk offset, chunk count) of rows whose LAST column is the element count; through pinned
    memory, asynchronously, like Adam._table"""
    tens = np.zeros((len(rows), len(rows[0])), dtype=np.int64)
    tens[:] = rows
    ct, co = [], []
    for k, r in enumerate(rows):
        n = -(-r[-1] // CHUNK)
        ct += [k] * n
        co += list(range(n))
    up = (lambda a: torch.from_numpy(a).pin_memory().to(dev, non_blocking=True)) if dev.type == "cuda" else (lambda a: torch.from_numpy(a).to(dev))
    return up(tens.view(np.uint8).reshape(-1)), up(np.asarray(ct, dtype=np.int32)), up(np.asarray(co, dtype=np.int32)), len(ct)


class EMA:
    """Exponential moving average of a model's parameters: ``e <- e + (p - e) (1 - d)`` after every optimiser step.

    ``EMA(module_or_named_parameters, decay=0.9999, *, warmup=True, update_after_step=0, update_every=1)``.  One fp32 shadow per parameter on
    the parameter's device, initialised as a copy.  The schedule is host state, in double: the s-th optimiser step (s = 1, 2, ...) updates
    only when ``s % update_every == 0``; such a step is a COPY (weight 1) while ``s <= update_after_step``, and otherwise the k-th averaging
    update (k = 1, 2, ...) with ``d_k = min(decay, (1 + k) / (10 + k))`` under ``warmup``, else ``decay``.

    Use it one of two ways, never both for the same step: call ``update()`` after ``optimizer.step()`` (one ``mi_ema_update`` launch for all
    eligible parameters -- fp32, contiguous, on the GPU -- and torch ops for the rest), or ``attach(optimizer)`` to an ``optim.Adam``, whose
    ``step()`` then advances the schedule itself and issues ``mi_adam_ema_step`` in place of ``mi_adam_step`` (no extra launch)."""

    def __init__(self, params, decay: float = 0.9999, *, warmup: bool = True, update_after_step: int = 0, update_every: int = 1):
        if not 0.0 <= decay < 1.0:
            raise ValueError(f"EMA decay must lie in [0, 1), got {decay}")
        if int(update_after_step) != update_after_step or update_after_step < 0:
            raise ValueError(f"EMA update_after_step must be a count >= 0, got {update_after_step}")
        if int(update_every) != update_every or update_every < 1:
            raise ValueError(f"EMA update_every must be a count >= 1, got {update_every}")
        named = list(params.named_parameters()) if isinstance(params, torch.nn.Module) else list(params)
        if not named or not all(isinstance(n, str) and torch.is_tensor(p) for n, p in named):
            raise ValueError("EMA needs a module or a non-empty iterable of (name, parameter)")
        if len({n for n, _ in named}) != len(named):
            raise ValueError("EMA: parameter names must be unique")
        self.decay, self.warmup = float(decay), bool(warmup)
        self.update_after_step, self.update_every = int(update_after_step), int(update_every)
        self.step = 0             # optimiser steps seen
        self.num_updates = 0      # averaging updates done (k of d_k)
        self.names = [n for n, _ in named]
        self.params = [p for _, p in named]
        with torch.no_grad():
            self.shadows = [p.detach().to(torch.float32, copy=True).contiguous() for p in self.params]
        self._shadow_of = dict(zip(self.params, self.shadows))
        self._tables = {}
        self._stash = None        # inside average_parameters(): the originals of the parameters the swap kernel does not take
        self._held = ()           # inside average_parameters(): the parameters whose buffer was exchanged with their shadow's

    # ------------------------------------------------------------------ schedule (host)
    def decay_at(self, k: int) -> float:
        """d_k of the k-th averaging update, k = 1, 2, ..."""
        return min(self.decay, (1.0 + k) / (10.0 + k)) if self.warmup else self.decay

    def advance(self):
        """Count one optimiser step and return the weight ``w = 1 - d`` of its shadow update: None when none is due, 1.0 for a copy.
        (``update()`` and an attached ``Adam.step()`` call this; it launches nothing.)"""
        self._not_inside("a shadow update")
        self.step += 1
        if self.step % self.update_every != 0:
            return None
        if self.step <= self.update_after_step:
            return 1.0
        self.num_updates += 1
        return 1.0 - self.decay_at(self.num_updates)

    def _not_inside(self, what: str):
        """inside average_parameters() the buffers are exchanged: the shadows hold the live weights, and an update would average the wrong way"""
        if self._stash is not None:
            raise RuntimeError(f"EMA: {what} inside average_parameters() -- the parameters hold the averages there; leave the block first")

    def _averages(self):
        """the tensors that hold the averages right now, in the order of ``names``: the shadows -- or, inside average_parameters(), the
        exchanged parameters' own buffers"""
        return [p.detach() if p in self._held else e for p, e in zip(self.params, self.shadows)]

    # ------------------------------------------------------------------ launches
    def _params(self, slot, ps, w: float) -> "L.MiEmaParams":
        """mi_ema_params over the parameters ``ps`` (table cached per slot, rebuilt only when a pointer changes)"""
        rows = tuple((self._shadow_of[p].data_ptr(), p.data_ptr(), p.numel()) for p in ps)
        tb = self._tables.get(slot)
        if tb is None or tb[0] != rows:
            if len(self._tables) >= 64:                     # (parameter sets that keep changing: nothing accumulates)
                self._tables.clear()
            tb = self._tables[slot] = (rows,) + _upload(rows, ps[0].device)
        a = L.MiEmaParams()
        a.tensors, a.chunk_tensor, a.chunk_off, a.nchunks, a.chunk, a.w = tb[1].data_ptr(), tb[2].data_ptr(), tb[3].data_ptr(), tb[4], CHUNK, w
        return a

    def _split(self, skip=()):
        """(eligible parameters per device, the others) among those not in ``skip``"""
        skip = set(skip)
        by_dev, rest = {}, []
        for p, e in zip(self.params, self.shadows):
            if p in skip:
                continue
            if p.numel() and _eligible(p, e):
                by_dev.setdefault(p.device, []).append(p)
            else:
                rest.append((p, e))
        return by_dev, rest

    @torch.no_grad()
    def _apply(self, w: float, skip=()):
        by_dev, rest = self._split(skip)
        for dev, ps in by_dev.items():
            a = self._params(("update", str(dev), len(ps)), ps, w)
            L.check(L.lib().mi_ema_update(C.byref(a), L.current_stream()), "mi_ema_update")
        for p, e in rest:                                   # the same formula in torch ops, in double, rounded once
            src = p.detach().to(device=e.device, dtype=torch.float64)
            e.copy_(src if w == 1.0 else torch.addcmul(e.double(), src - e.double(), torch.tensor(w, dtype=torch.float64, device=e.device)))

    def update(self):
        """The shadow update of one optimiser step (not for an attached EMA: the optimiser's ``step()`` does it)."""
        w = self.advance()
        if w is not None:
            self._apply(w)

    def attach(self, optimizer):
        """Fold the shadow update into ``optimizer.step()`` (an ``optim.Adam``): on steps where an update is due, one ``mi_adam_ema_step``
        per launch the optimiser would issue anyway; parameters that took no gradient, or Adam's slow path, through ``mi_ema_update`` / torch.
        A launch is fused only when EVERY parameter in it has a shadow here, on its own device: an EMA over part of what the optimiser steps
        (one U-Net of a cascade the optimiser holds whole) gets correct shadows from ``mi_adam_step`` plus one ``mi_ema_update``, not the
        fused kernel -- give the optimiser one parameter group per averaged part, or average everything it steps."""
        if not isinstance(optimizer, Adam):
            raise TypeError("EMA.attach needs a minimagen_amd.optim.Adam; call update() after the step of any other optimiser")
        if optimizer._ema is not None and optimizer._ema is not self:
            raise ValueError("this optimiser already has an EMA attached")
        optimizer._ema = self
        return self

    def detach(self, optimizer):
        if optimizer._ema is self:
            optimizer._ema = None

    # ------------------------------------------------------------------ using the averages
    def _drain(self):
        for dev in {p.device for p in self.params if p.is_cuda}:
            torch.cuda.synchronize(dev)

    @torch.no_grad()
    def _swap(self):
        by_dev, rest = self._split()
        for dev, ps in by_dev.items():
            a = self._params(("swap", str(dev)), ps, 0.0)
            L.check(L.lib().mi_ema_swap(C.byref(a), L.current_stream()), "mi_ema_swap")
            for p in ps:                                    # written through raw pointers: tell autograd / every version-keyed cache
                torch.autograd.graph.increment_version(p)
        return [p for ps in by_dev.values() for p in ps], rest

    @contextmanager
    def average_parameters(self):
        """``with ema.average_parameters():`` -- the parameters hold the averages inside the block (validation, sampling, saving) and
        their own values again after it.  A validation-cadence operation, not a per-step one: entry and exit each DRAIN THE DEVICE
        (``sample(_async=True)`` calls in flight read the weights from stage streams that the caller's stream does not order), exchange
        parameters and shadows with one ``mi_ema_swap`` launch, and bump every parameter's version counter, so the U-Net engines and the
        training path re-pack their weight copies on the next call (twice per block).  Inside, ``state_dict()`` and ``copy_to()`` still
        give the averages; a shadow update (``update()``, the ``step()`` of an attached optimiser) and ``load_state_dict()`` raise
        ``RuntimeError``: the shadows' buffers hold the live weights there."""
        if self._stash is not None:
            raise RuntimeError("EMA.average_parameters() does not nest")
        self._drain()
        swapped, rest = self._swap()
        with torch.no_grad():
            self._held = frozenset(swapped)
            self._stash = [(p, p.detach().clone()) for p, _ in rest]      # (no bit-exact exchange with an fp32 shadow for these: keep the originals)
            for p, e in rest:
                p.copy_(e.to(device=p.device, dtype=p.dtype))
        try:
            yield self
        finally:
            self._drain()
            self._swap()
            with torch.no_grad():
                for p, keep in self._stash:
                    p.copy_(keep)
            self._stash, self._held = None, ()

    @torch.no_grad()
    def copy_to(self, module: torch.nn.Module):
        """write the averages into the parameters of the same names of another module (a second model kept for sampling)"""
        by_name = dict(zip(self.names, self._averages()))
        target = dict(module.named_parameters())
        missing = [n for n in by_name if n not in target]
        if missing:
            raise KeyError(f"EMA.copy_to: the module has no parameter named {missing[0]!r}" + (f" (and {len(missing) - 1} more)" if len(missing) > 1 else ""))
        for n, e in by_name.items():
            target[n].copy_(e.to(device=target[n].device, dtype=target[n].dtype))

    def state_dict(self):
        """counters, hyper-parameters and the averages by name (the averages also when taken inside average_parameters())"""
        return dict(decay=self.decay, warmup=self.warmup, update_after_step=self.update_after_step, update_every=self.update_every,
                    step=self.step, num_updates=self.num_updates, shadows={n: e.detach().clone() for n, e in zip(self.names, self._averages())})

    @torch.no_grad()
    def load_state_dict(self, state):
        self._not_inside("load_state_dict()")
        sh = state["shadows"]
        if set(sh) != set(self.names):
            raise KeyError("EMA.load_state_dict: the shadows' names do not match this EMA's parameters")
        for n, e in zip(self.names, self.shadows):
            if tuple(sh[n].shape) != tuple(e.shape):
                raise ValueError(f"EMA.load_state_dict: shadow {n!r} has shape {tuple(sh[n].shape)}, expected {tuple(e.shape)}")
        decay, every, after = float(state["decay"]), int(state["update_every"]), int(state["update_after_step"])
        if not 0.0 <= decay < 1.0 or every < 1 or after < 0 or int(state["step"]) < 0 or int(state["num_updates"]) < 0:
            raise ValueError("EMA.load_state_dict: invalid hyper-parameters / counters")
        for n, e in zip(self.names, self.shadows):
            e.copy_(sh[n])                                  # in place: the cached tables keep their pointers
        self.decay, self.warmup, self.update_every, self.update_after_step = decay, bool(state["warmup"]), every, after
        self.step, self.num_updates = int(state["step"]), int(state["num_updates"])
