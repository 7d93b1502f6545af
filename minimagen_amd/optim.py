"""``Adam`` with torch.optim.Adam's constructor, state layout and update (the optimiser of the reference's train.py:99-100), whose step
is ONE launch of the multi-tensor HIP kernel ``mi_adam_step`` (csrc/optim.hip) for all parameters on the GPU.

State per parameter: ``step`` (a host float tensor like torch's default), ``exp_avg``, ``exp_avg_sq`` -- a ``state_dict()`` of either
optimiser loads into the other.  Parameters that are not fp32 / not on the GPU / not contiguous take torch's own update.

``EMA`` keeps an exponential moving average of the parameters: one fp32 shadow per parameter, updated by ``mi_ema_update`` -- or,
attached to an ``Adam``, inside that optimiser's launch (``mi_adam_ema_step``) -- and exchanged with the live weights by ``mi_ema_swap`` for
validation and sampling (``average_parameters()``)."""
from __future__ import annotations

import ctypes as C
from contextlib import contextmanager

import numpy as np
import torch

from . import _lib as L

CHUNK = 4096           # elements per launched workgroup


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0., amsgrad: bool = False,
                 maximize: bool = False, capturable: bool = False):
        if amsgrad or maximize or capturable:
            raise NotImplementedError("minimagen_amd.optim.Adam implements torch.optim.Adam's default update only (no amsgrad / maximize / capturable)")
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0 or not 0.0 <= weight_decay:
            raise ValueError("invalid Adam hyper-parameters")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._tables = {}
        self._count = {}          # parameter -> step count as a Python int (mirrored into the state's host ``step`` tensor at every step)
        self._ema = None          # an EMA whose shadow update rides in this optimiser's launch (EMA.attach)

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
        for gi, group in enumerate(self.param_groups):
            b1, b2 = group["betas"]
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
            for slot, (t, ps) in enumerate(by_step.items()):
                _, tens, ct, co, nchunks = self._table((gi, slot), ps)
                a = L.MiAdamParams()
                a.tensors, a.chunk_tensor, a.chunk_off, a.nchunks, a.chunk = tens.data_ptr(), ct.data_ptr(), co.data_ptr(), nchunks, CHUNK
                a.lr, a.beta1, a.beta2, a.eps, a.weight_decay = group["lr"], b1, b2, group["eps"], group["weight_decay"]
                a.bias_correction1, a.bias_correction2 = 1.0 - b1 ** t, 1.0 - b2 ** t
                a.one_minus_beta1, a.one_minus_beta2 = 1.0 - b1, 1.0 - b2
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
                g = p.grad if group["weight_decay"] == 0 else p.grad.add(p, alpha=group["weight_decay"])
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
