"""Gradient-norm clipping on the device: the three kernels (mi_grad_sumsq, mi_grad_clip_coef, mi_grad_scale), ``optim.clip_grad_norm_``
(in place), ``optim.Adam(max_grad_norm=...)`` (deferred: the Adam launch reads the coefficient) and ``MinimagenTrain(grad_clip="device")``."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from minimagen_amd import _lib as L
from tests._backend import BACKENDS, setup

SHAPES = [(1,), (16,), (255,), (256,), (257,), (4095,), (4096,), (4097,), (5000,), (33, 129), (16, 8, 3, 3), (3, 4096)]
CHUNK = 4096


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def spread(shape, gen):
    """fp32 values of either sign with magnitudes 2^-20 ... 2^10"""
    return (torch.rand(shape, generator=gen) * 2 - 1).sign() * torch.exp2(torch.rand(shape, generator=gen) * 30 - 20)


def grad_set(dev, gen):
    """(host copies, device gradients): SHAPES and one [1:] slice of a 4098-element buffer -- contiguous, 4-byte aligned only"""
    host = [spread(s, gen) for s in SHAPES]
    buf = spread((4098,), gen)
    on_dev = [t.clone().to(dev) for t in host]
    sliced = buf.clone().to(dev)[1:]
    assert sliced.is_contiguous() and sliced.data_ptr() % 16 == 4
    return host + [buf[1:].clone()], on_dev + [sliced]


def grad_block(gs, dev, grad_scale=None):
    """(mi_adam_params over gradients alone: p / m / v NULL, no scalar set; tensors to keep alive)"""
    from minimagen_amd.optim import _upload
    tens, ct, co, n = _upload([(0, g.data_ptr(), 0, 0, g.numel()) for g in gs], dev)
    a = L.MiAdamParams()
    a.tensors, a.chunk_tensor, a.chunk_off, a.nchunks, a.chunk = tens.data_ptr(), ct.data_ptr(), co.data_ptr(), n, CHUNK
    a.grad_scale = grad_scale
    return a, (tens, ct, co)


def sumsq64(ts):
    """the exact squares of fp32 values, summed without error"""
    return math.fsum(float(x) for t in ts for x in t.detach().cpu().reshape(-1).double().pow(2).tolist())


def coef64(norm, max_norm):
    return min(1.0, max_norm / (norm + 1e-6))


def params_with(grads):
    ps = [torch.nn.Parameter(torch.zeros(g.shape, dtype=g.dtype, device=g.device)) for g in grads]
    for p, g in zip(ps, grads):
        p.grad = g
    return ps


# ------------------------------------------------------------------------------------------------ 1. mi_grad_sumsq
@pytest.mark.parametrize("backend", BACKENDS)
def test_grad_sumsq_against_fp64(backend):
    """every partials[c] against the exact sum of that chunk's squares: the products are exact in fp64 (24 x 24 bits), and at most 4096
    additions round, 2^-53 relative each -> |d| <= 4096 2^-52 ref with room; the gradients are only read; a second launch repeats the bits"""
    dev = setup(backend)
    host, gs = grad_set(dev, torch.Generator().manual_seed(21))
    a, keep = grad_block(gs, dev)
    partials = torch.full((a.nchunks + 1,), float("nan"), dtype=torch.float64, device=dev)
    L.check(L.lib().mi_grad_sumsq(C.byref(a), partials.data_ptr(), L.current_stream()), "mi_grad_sumsq")
    first = partials.cpu().clone()
    L.check(L.lib().mi_grad_sumsq(C.byref(a), partials.data_ptr(), L.current_stream()), "mi_grad_sumsq")
    second = partials.cpu()
    assert torch.equal(first[:-1].view(torch.int64), second[:-1].view(torch.int64)) and math.isnan(float(second[-1]))   # (nothing past nchunks)
    c, worst = 0, 0.0
    for h in host:
        flat = h.reshape(-1)
        for o in range(0, flat.numel(), CHUNK):
            ref = sumsq64([flat[o:o + CHUNK]])
            err = abs(float(first[c]) - ref)
            worst = max(worst, err / (4096 * 2.0 ** -52 * ref))
            assert err <= 4096 * 2.0 ** -52 * ref, (tuple(h.shape), o, float(first[c]), ref)
            c += 1
    assert c == a.nchunks
    for h, g in zip(host, gs):
        assert same_bits(g, h)
    print(f"mi_grad_sumsq: {c} chunks, worst error / bound = {worst:.2e}")


# ------------------------------------------------------------------------------------------------ 2. mi_grad_clip_coef
def _coef(lib, dev, partials, extra, max_norm):
    out = torch.full((3,), -7.0, device=dev)
    n = 0 if partials is None else partials.numel()
    L.check(lib.mi_grad_clip_coef(partials.data_ptr() if n else None, n, extra.data_ptr() if extra is not None else None, max_norm, out.data_ptr(),
                                  L.current_stream()), "mi_grad_clip_coef")
    o = out.cpu()
    assert float(o[2]) == -7.0
    return o[:2]


@pytest.mark.parametrize("backend", BACKENDS)
def test_grad_clip_coef_on_synthetic_partials(backend):
    """out[0] = (float) sqrt(S), out[1] = (float) min(1, max_norm / (sqrt(S) + 1e-6)): one rounding to float (2^-24 relative) on top of an
    fp64 summation error far below it -> both within 2^-23 relative"""
    dev = setup(backend)
    lib = L.lib()
    gen = torch.Generator().manual_seed(22)
    tol = 2.0 ** -23
    for n in (0, 1, 255, 256, 257, 1000, 4096, 4097, 5000):
        for with_extra in ((True,) if n == 0 else (False, True)):
            host = torch.rand(n, generator=gen, dtype=torch.float64) * 100.0 + 1e-3
            hx = torch.rand((), generator=gen, dtype=torch.float64) * 50.0 + 1e-3 if with_extra else None
            S = math.fsum(host.tolist() + ([float(hx)] if with_extra else []))
            norm = math.sqrt(S)
            partials, extra = (host.to(dev) if n else None), (hx.to(dev) if with_extra else None)
            for max_norm in (float(np.float32(norm / 3.0)), float(np.float32(norm * 0.999)), float(np.float32(norm * 2.0)), 0.0):
                o = _coef(lib, dev, partials, extra, max_norm)
                want = coef64(norm, max_norm)
                assert abs(float(o[0]) - norm) <= tol * norm, (n, with_extra, float(o[0]), norm)
                assert abs(float(o[1]) - want) <= tol * want, (n, with_extra, max_norm, float(o[1]), want)
                if max_norm > norm:
                    assert float(o[1]) == 1.0                        # exactly: mi_grad_scale's early exit and Adam's g * 1.0f depend on it
                if max_norm == 0.0:
                    assert float(o[1]) == 0.0
                assert same_bits(_coef(lib, dev, partials, extra, max_norm), o)
    zeros = torch.zeros(300, dtype=torch.float64, device=dev)
    assert _coef(lib, dev, zeros, None, 50.0).tolist() == [0.0, 1.0]
    assert _coef(lib, dev, zeros, zeros[:1].reshape(()), 50.0).tolist() == [0.0, 1.0]
    for n in (300, 5000):
        bad = torch.rand(n, generator=gen, dtype=torch.float64)
        bad[n // 2] = float("inf")
        assert _coef(lib, dev, bad.to(dev), None, 50.0).tolist() == [float("inf"), 0.0]
        bad[n // 2] = float("nan")
        o = _coef(lib, dev, bad.to(dev), None, 50.0)
        assert math.isnan(float(o[0])) and math.isnan(float(o[1]))
    o = _coef(lib, dev, zeros, torch.tensor(float("nan"), dtype=torch.float64, device=dev), 50.0)
    assert math.isnan(float(o[0])) and math.isnan(float(o[1]))


@pytest.mark.parametrize("backend", BACKENDS)
def test_grad_entries_reject_bad_arguments(backend):
    dev = setup(backend)
    lib, st = L.lib(), L.current_stream()
    g = torch.ones(8, device=dev)
    scale = torch.full((1,), 0.5, device=dev)
    good, keep = grad_block([g], dev, scale.data_ptr())
    partials = torch.full((4,), 3.0, dtype=torch.float64, device=dev)
    out = torch.full((2,), -7.0, device=dev)

    def variant(**kw):
        b = L.MiAdamParams.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(b, k, v)
        return b
    for b in (variant(nchunks=0), variant(chunk=0), variant(tensors=None), variant(chunk_tensor=None), variant(chunk_off=None)):
        assert lib.mi_grad_sumsq(C.byref(b), partials.data_ptr(), st) == -1 and b"mi_grad_sumsq: empty / missing tables" in lib.mi_last_error()
        assert lib.mi_grad_scale(C.byref(b), st) == -1 and b"mi_grad_scale: empty / missing tables" in lib.mi_last_error()
    assert lib.mi_grad_sumsq(None, partials.data_ptr(), st) == -1 and b"mi_grad_sumsq" in lib.mi_last_error()
    assert lib.mi_grad_sumsq(C.byref(good), None, st) == -1 and b"mi_grad_sumsq: NULL partials" in lib.mi_last_error()
    assert lib.mi_grad_scale(None, st) == -1 and b"mi_grad_scale" in lib.mi_last_error()
    assert lib.mi_grad_scale(C.byref(variant(grad_scale=None)), st) == -1 and b"mi_grad_scale: NULL grad_scale" in lib.mi_last_error()
    x = partials[:1].reshape(())
    for args, msg in (((partials.data_ptr(), 4, None, 50.0, None), b"NULL out"), ((partials.data_ptr(), -1, None, 50.0, out.data_ptr()), b"negative"),
                      ((None, 4, None, 50.0, out.data_ptr()), b"NULL partials"), ((None, 4, x.data_ptr(), 50.0, out.data_ptr()), b"NULL partials"),
                      ((None, 0, None, 50.0, out.data_ptr()), b"nothing to sum"), ((partials.data_ptr(), 0, None, 50.0, out.data_ptr()), b"nothing to sum"),
                      ((partials.data_ptr(), 4, None, -1.0, out.data_ptr()), b"max_norm"), ((partials.data_ptr(), 4, None, float("nan"), out.data_ptr()), b"max_norm")):
        assert lib.mi_grad_clip_coef(*args, st) == -1 and b"mi_grad_clip_coef" in lib.mi_last_error() and msg in lib.mi_last_error(), msg
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert torch.equal(g.cpu(), torch.ones(8)) and out.cpu().tolist() == [-7.0, -7.0] and partials.cpu().tolist() == [3.0] * 4      # nothing was launched


# ------------------------------------------------------------------------------------------------ 3. optim.clip_grad_norm_
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("max_norm", [50, 1e-3, 1e9])
def test_clip_grad_norm_against_fp64(backend, max_norm):
    """norm within 2^-23 relative of the double norm (one rounding to float); every element within 2^-22 |g coef64| of g coef64: one
    rounding of the coefficient and one of the product, 2^-24 each (and max_norm's own to a float)"""
    from minimagen_amd.optim import clip_grad_norm_
    dev = setup(backend)
    host, gs = grad_set(dev, torch.Generator().manual_seed(23))
    ps = params_with(gs)
    versions = [g._version for g in gs]
    total = clip_grad_norm_(ps, max_norm)
    norm = math.sqrt(sumsq64(host))
    coef = coef64(norm, float(max_norm))
    assert total.dim() == 0 and total.dtype == torch.float32 and total.device == gs[0].device
    assert abs(float(total) - norm) <= 2.0 ** -23 * norm, (float(total), norm)
    theirs = [torch.nn.Parameter(torch.zeros_like(h)) for h in host]
    for p, h in zip(theirs, host):
        p.grad = h.clone()
    torch.nn.utils.clip_grad_norm_(theirs, max_norm)
    ours_worst = torch_worst = 0.0
    for h, g, p, v in zip(host, gs, ps, versions):
        assert p.grad is g and g._version > v
        ref = h.double() * coef
        err = (g.cpu().double() - ref).abs()
        ours_worst = max(ours_worst, float((err / ref.abs()).max()))
        assert (err <= 2.0 ** -22 * ref.abs()).all(), (tuple(h.shape), float((err / ref.abs()).max()) / 2.0 ** -23)
        if max_norm == 1e9:
            assert same_bits(g, h)
    for h, p in zip(host, theirs):
        ref = h.double() * coef
        torch_worst = max(torch_worst, float(((p.grad.double() - ref).abs() / ref.abs()).max()))
    print(f"clip_grad_norm_ max_norm={max_norm}: coef {coef:.3e}; worst element deviation / 2^-23: ours {ours_worst / 2.0 ** -23:.2f}, "
          f"torch's fp32 function {torch_worst / 2.0 ** -23:.2f} (information)")


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("value", [1e30, 1e-30])
def test_clip_grad_norm_beyond_fp32_squares(backend, value):
    """|g| = 1e30 and 1e-30: the squares overflow / vanish in fp32 (an fp32 accumulation answers inf / 0); in fp64 the norm is finite, non-zero
    and within the same bounds"""
    from minimagen_amd.optim import clip_grad_norm_
    dev = setup(backend)
    gen = torch.Generator().manual_seed(24)
    host = [(torch.rand(s, generator=gen) + 0.5) * value * (torch.rand(s, generator=gen) * 2 - 1).sign() for s in [(5000,), (33, 129), (7,)]]
    gs = [h.clone().to(dev) for h in host]
    total = clip_grad_norm_(params_with(gs), 50)
    norm = math.sqrt(sumsq64(host))
    coef = coef64(norm, 50.0)
    assert math.isfinite(float(total)) and float(total) != 0.0 and abs(float(total) - norm) <= 2.0 ** -23 * norm, (float(total), norm)
    assert float(torch.stack([h.pow(2).sum() for h in host]).sum().sqrt()) in (float("inf"), 0.0)       # what an fp32 accumulation answers
    for h, g in zip(host, gs):
        ref = h.double() * coef
        assert ((g.cpu().double() - ref).abs() <= 2.0 ** -22 * ref.abs()).all() and (g != 0).all()


@pytest.mark.parametrize("backend", BACKENDS)
def test_clip_grad_norm_nonfinite(backend):
    """torch's behaviour: a NaN element makes every gradient NaN; an inf element makes the coefficient 0 -- that element inf * 0 = NaN, the
    rest 0; error_if_nonfinite raises before anything is scaled"""
    from minimagen_amd.optim import clip_grad_norm_
    dev = setup(backend)
    for bad in (float("nan"), float("inf")):
        host, gs = grad_set(dev, torch.Generator().manual_seed(25))
        host[8].view(-1)[4321] = bad
        gs[8].view(-1)[4321] = bad
        ps = params_with(gs)
        with pytest.raises(RuntimeError, match="non-finite"):
            clip_grad_norm_(ps, 50, error_if_nonfinite=True)
        assert all(same_bits(g, h) for g, h in zip(gs, host))
        total = clip_grad_norm_(ps, 50)
        if math.isnan(bad):
            assert math.isnan(float(total)) and all(bool(g.isnan().all()) for g in gs)
        else:
            assert float(total) == float("inf") and bool(gs[8].view(-1)[4321].isnan())
            for k, g in enumerate(gs):
                flat = g.reshape(-1).cpu()
                keep = torch.ones(flat.numel(), dtype=torch.bool)
                if k == 8:
                    keep[4321] = False
                assert (flat[keep] == 0).all()


@pytest.mark.parametrize("backend", BACKENDS)
def test_clip_grad_norm_mixed_and_delegated(backend):
    from minimagen_amd.optim import clip_grad_norm_
    dev = setup(backend)
    gen = torch.Generator().manual_seed(26)
    # one fp64 parameter and one non-contiguous gradient among the others: the same norm, the same coefficient
    host, gs = grad_set(dev, gen)
    h64 = spread((7, 5), gen).double() * 3.0
    hnc = spread((6, 5), gen)
    g64 = h64.clone().to(dev)
    gnc = hnc.t().contiguous().to(dev).t()
    assert not gnc.is_contiguous() and torch.equal(gnc.cpu(), hnc)
    ps = params_with(gs + [g64, gnc])
    assert ps[-1].grad is gnc and ps[-2].grad.dtype == torch.float64
    total = clip_grad_norm_(ps, 50)
    norm = math.sqrt(math.fsum([sumsq64(host), sumsq64([hnc]), math.fsum((h64.reshape(-1) ** 2).tolist())]))
    coef = coef64(norm, 50.0)
    assert coef < 1.0 and abs(float(total) - norm) <= 2.0 ** -23 * norm
    for h, g in zip(host + [h64, hnc], gs + [g64, gnc]):
        ref = h.double() * coef
        assert ((g.cpu().double() - ref).abs() <= 2.0 ** -22 * ref.abs()).all(), tuple(h.shape)
    # other norms: torch's function, torch's value
    for norm_type in (float("inf"), 1):
        host, gs = grad_set(dev, gen)
        theirs = params_with([g.clone() for g in gs])
        mine = params_with(gs)
        a, b = clip_grad_norm_(mine, 50, norm_type=norm_type), torch.nn.utils.clip_grad_norm_(theirs, 50, norm_type=norm_type)
        assert same_bits(a, b) and all(same_bits(p.grad, q.grad) for p, q in zip(mine, theirs))
    # nothing to clip
    zero = clip_grad_norm_([], 50)
    assert torch.is_tensor(zero) and float(zero) == 0.0
    assert float(clip_grad_norm_([torch.nn.Parameter(torch.ones(3, device=dev))], 50)) == 0.0
    # a single tensor, as torch allows
    p = torch.nn.Parameter(torch.zeros(5000, device=dev))
    p.grad = torch.full((5000,), 2.0, device=dev)
    v = p.grad._version
    assert abs(float(clip_grad_norm_(p, 1.0)) - 2.0 * math.sqrt(5000)) < 1e-4 and p.grad._version > v
    assert abs(float(p.grad.double().pow(2).sum().sqrt()) - 1.0) < 1e-6
    with pytest.raises(ValueError):
        clip_grad_norm_(p, -1.0)


# ------------------------------------------------------------------------------------------------ 4. Adam(max_grad_norm=...)
ADAM_SHAPES = [(16, 8, 3, 3), (16,), (5000,), (3, 7), (1,), (33, 129)]      # tests/test_training_loop.py::test_adam_kernel_matches_torch_adam
GROUP_KW = [dict(lr=1e-2, weight_decay=0.0), dict(lr=3e-3, weight_decay=0.01)]


def _groups(ps):
    return [dict(params=ps[:4]), dict(params=ps[4:], weight_decay=0.01, lr=3e-3)]


def _fresh_grads(step, gen):
    """gradient k at scale 10^(k - 3); parameter 3 gets none on odd steps (its own step count)"""
    return [None if (k == 3 and step % 2) else torch.randn(s, generator=gen) * (10.0 ** (k - 3)) for k, s in enumerate(ADAM_SHAPES)]


class HandRun:
    """the launches Adam(max_grad_norm=...) is specified to issue, by hand: mi_grad_sumsq per (group, step count) table into slices of one
    partials buffer -> mi_grad_clip_coef -> mi_adam_step (or mi_adam_ema_step) with grad_scale at the coefficient"""

    def __init__(self, base, dev, max_norm, shadows=False):
        self.dev, self.max_norm = dev, max_norm
        self.p = [b.clone().to(dev) for b in base]
        self.m, self.v = [torch.zeros_like(p) for p in self.p], [torch.zeros_like(p) for p in self.p]
        self.e = [p.clone() for p in self.p] if shadows else None
        self.count = [0] * len(base)
        self.updates = 0

    def step(self, grads):
        from minimagen_amd.optim import _upload
        lib, st, dev = L.lib(), L.current_stream(), self.dev
        gs = [None if g is None else g.clone().to(dev) for g in grads]
        tables = []
        for lo, hi, kw in ((0, 4, GROUP_KW[0]), (4, 6, GROUP_KW[1])):
            by_count = {}
            for k in range(lo, hi):
                if gs[k] is not None:
                    self.count[k] += 1
                    by_count.setdefault(self.count[k], []).append(k)
            tables += [(t, ks, kw) for t, ks in by_count.items()]
        blocks, keep = [], []
        for t, ks, kw in tables:
            tens, ct, co, n = _upload([(self.p[k].data_ptr(), gs[k].data_ptr(), self.m[k].data_ptr(), self.v[k].data_ptr(), self.p[k].numel()) for k in ks], dev)
            a = L.MiAdamParams()
            a.tensors, a.chunk_tensor, a.chunk_off, a.nchunks, a.chunk = tens.data_ptr(), ct.data_ptr(), co.data_ptr(), n, CHUNK
            a.lr, a.beta1, a.beta2, a.eps, a.weight_decay = kw["lr"], 0.9, 0.999, 1e-8, kw["weight_decay"]
            a.bias_correction1, a.bias_correction2, a.one_minus_beta1, a.one_minus_beta2 = 1.0 - 0.9 ** float(t), 1.0 - 0.999 ** float(t), 1.0 - 0.9, 1.0 - 0.999
            blocks.append(a), keep.append((tens, ct, co))
        partials = torch.empty(sum(a.nchunks for a in blocks), dtype=torch.float64, device=dev)
        at = 0
        for a in blocks:
            L.check(lib.mi_grad_sumsq(C.byref(a), partials.data_ptr() + 8 * at, st), "mi_grad_sumsq")
            at += a.nchunks
        out = torch.empty(2, device=dev)
        L.check(lib.mi_grad_clip_coef(partials.data_ptr(), partials.numel(), None, self.max_norm, out.data_ptr(), st), "mi_grad_clip_coef")
        w = None
        if self.e is not None:                                   # EMA(decay=0.9): the k-th update averages with d_k = min(0.9, (1 + k) / (10 + k))
            self.updates += 1
            w = 1.0 - min(0.9, (1.0 + self.updates) / (10.0 + self.updates))
        for a, (t, ks, kw) in zip(blocks, tables):
            a.grad_scale = out.data_ptr() + 4
            if w is None:
                L.check(lib.mi_adam_step(C.byref(a), st), "mi_adam_step")
            else:
                e, keep_e = self._ema_block(ks, w)
                L.check(lib.mi_adam_ema_step(C.byref(a), C.byref(e), st), "mi_adam_ema_step")
        rest = [k for k in range(len(gs)) if gs[k] is None]
        if w is not None and rest:                               # no gradient at this step: the shadow still follows the (unchanged) parameter
            e, keep_e = self._ema_block(rest, w)
            L.check(lib.mi_ema_update(C.byref(e), st), "mi_ema_update")
        if dev.type == "cuda":
            torch.cuda.synchronize()
        return out.cpu()

    def _ema_block(self, ks, w):
        from minimagen_amd.optim import _upload
        tens, ct, co, n = _upload([(self.e[k].data_ptr(), self.p[k].data_ptr(), self.p[k].numel()) for k in ks], self.dev)
        a = L.MiEmaParams()
        a.tensors, a.chunk_tensor, a.chunk_off, a.nchunks, a.chunk, a.w = tens.data_ptr(), ct.data_ptr(), co.data_ptr(), n, CHUNK, w
        return a, (tens, ct, co)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("max_norm", [50, 0.5, 1e6])
def test_adam_max_grad_norm(backend, max_norm):
    """six steps, two groups, a parameter that skips every other step: (a) the bits of the hand-run launches, (b) gradients untouched,
    (c) grad_norm within 2^-23 of the double norm, (d) torch's clip + torch.optim.Adam within test_adam_kernel_matches_torch_adam's
    2e-6 max(1, max|p|), (e) never clipping = no keyword, bit for bit, (f) the state dict knows nothing of it"""
    from minimagen_amd.optim import Adam
    dev = setup(backend)
    gen = torch.Generator().manual_seed(3)
    base = [torch.randn(s, generator=gen) for s in ADAM_SHAPES]
    mine = [torch.nn.Parameter(b.clone().to(dev)) for b in base]
    plain = [torch.nn.Parameter(b.clone().to(dev)) for b in base]
    ref = [torch.nn.Parameter(b.clone()) for b in base]
    om, op, orf = Adam(_groups(mine), lr=1e-2, max_grad_norm=max_norm), Adam(_groups(plain), lr=1e-2), torch.optim.Adam(_groups(ref), lr=1e-2, foreach=False)
    hand = HandRun(base, dev, float(max_norm))
    assert om.grad_norm is None and om.max_grad_norm == float(max_norm) and op.max_grad_norm is None
    norms = []
    for step in range(6):
        grads = _fresh_grads(step, gen)
        for k, g in enumerate(grads):
            for ps, d in ((mine, dev), (plain, dev), (ref, "cpu")):
                ps[k].grad = None if g is None else g.clone().to(d)
        om.step(); op.step()
        torch.nn.utils.clip_grad_norm_(ref, max_norm)
        orf.step()
        out = hand.step(grads)
        norm = math.sqrt(sumsq64([g for g in grads if g is not None]))
        assert (coef64(norm, float(max_norm)) < 1.0) == (max_norm != 1e6)                    # 50 and 0.5 clip at every step, 1e6 never
        assert om.grad_norm.dim() == 0 and om.grad_norm.device == mine[0].device and abs(float(om.grad_norm) - norm) <= 2.0 ** -23 * norm      # (c)
        assert float(om.grad_norm) == float(out[0])
        norms.append(om.grad_norm)
        for k, (p, g) in enumerate(zip(mine, grads)):
            assert (p.grad is None) == (g is None) and (g is None or same_bits(p.grad, g)), (step, k)                                          # (b)
            assert same_bits(p, hand.p[k]), (step, k)                                                                                           # (a)
            if p in om.state:
                assert same_bits(om.state[p]["exp_avg"], hand.m[k]) and same_bits(om.state[p]["exp_avg_sq"], hand.v[k]), (step, k)
    assert len({n.data_ptr() for n in norms}) == 6 and len({float(n) for n in norms}) == 6          # a fresh tensor per step: earlier ones keep their value
    for a, b, c in zip(mine, ref, plain):
        assert (a.detach().cpu() - b.detach()).abs().max() < 2e-6 * max(1.0, float(b.detach().abs().max())), tuple(a.shape)                     # (d)
        assert same_bits(a, c) == (max_norm == 1e6), tuple(a.shape)                                                                             # (e)
    sd = om.state_dict()                                                                                                                       # (f)
    assert "max_grad_norm" not in sd and all("max_grad_norm" not in g for g in sd["param_groups"]) and "grad_norm" not in sd
    assert [sorted(g) for g in sd["param_groups"]] == [sorted(g) for g in op.state_dict()["param_groups"]]
    o2 = torch.optim.Adam(_groups([torch.nn.Parameter(a.detach().cpu().clone()) for a in mine]), lr=1e-2, foreach=False)
    o2.load_state_dict({"state": {k: {n: (v.cpu() if torch.is_tensor(v) else v) for n, v in s.items()} for k, s in sd["state"].items()},
                        "param_groups": orf.state_dict()["param_groups"]})
    with pytest.raises(ValueError):
        Adam(_groups(plain), max_grad_norm=-1.0)
    with pytest.raises(TypeError):
        Adam(_groups(plain), 1e-2, (0.9, 0.999), 1e-8, 0., False, False, False, 50.0)        # keyword-only


@pytest.mark.parametrize("backend", BACKENDS)
def test_adam_max_grad_norm_with_ema_and_slow_path(backend):
    """(g) an attached EMA: parameters and shadows with the bits of the hand-run sequence ending in mi_adam_ema_step; and a float64
    parameter (Adam's slow path) enters the same global norm and takes the same coefficient"""
    from minimagen_amd.optim import Adam, EMA
    dev = setup(backend)
    gen = torch.Generator().manual_seed(3)
    base = [torch.randn(s, generator=gen) for s in ADAM_SHAPES]
    mine = [torch.nn.Parameter(b.clone().to(dev)) for b in base]
    om = Adam(_groups(mine), lr=1e-2, max_grad_norm=50)
    ema = EMA([(f"p{k}", p) for k, p in enumerate(mine)], decay=0.9).attach(om)
    hand = HandRun(base, dev, 50.0, shadows=True)
    for step in range(6):
        grads = _fresh_grads(step, gen)
        for k, g in enumerate(grads):
            mine[k].grad = None if g is None else g.clone().to(dev)
        om.step()
        hand.step(grads)
        for k in range(len(mine)):
            assert same_bits(mine[k], hand.p[k]) and same_bits(ema.shadows[k], hand.e[k]), (step, k)
    assert (ema.step, ema.num_updates) == (6, 6) and not same_bits(ema.shadows[0], mine[0])
    # slow path: fp64 parameter + fp32 parameters against torch's clip + Adam on CPU copies
    b32, b64 = torch.randn(5000, generator=gen), torch.randn(7, 5, generator=gen).double()
    g32, g64 = torch.randn(5000, generator=gen), torch.randn(7, 5, generator=gen).double() * 30.0
    ps = [torch.nn.Parameter(b32.clone().to(dev)), torch.nn.Parameter(b64.clone().to(dev))]
    rs = [torch.nn.Parameter(b32.clone()), torch.nn.Parameter(b64.clone())]
    for p, r, g in zip(ps, rs, (g32, g64)):
        p.grad, r.grad = g.clone().to(dev), g.clone()
    o, orf = Adam(ps, lr=1e-2, max_grad_norm=50), torch.optim.Adam(rs, lr=1e-2, foreach=False)
    o.step()
    torch.nn.utils.clip_grad_norm_(rs, 50)
    orf.step()
    norm = math.sqrt(math.fsum([sumsq64([g32]), math.fsum((g64.reshape(-1) ** 2).tolist())]))
    assert norm > 50 and abs(float(o.grad_norm) - norm) <= 2.0 ** -23 * norm
    assert same_bits(ps[1].grad, g64)
    for p, r in zip(ps, rs):
        assert (p.detach().cpu() - r.detach()).abs().max() < 2e-6 * max(1.0, float(r.abs().max()))
        assert (o.state[p]["exp_avg"].cpu() - orf.state[r]["exp_avg"]).abs().max() < 1e-6 * float(orf.state[r]["exp_avg"].abs().max())


# ------------------------------------------------------------------------------------------------ 5. the training loop
@pytest.mark.parametrize("backend", BACKENDS)
def test_train_flow_with_device_clip(backend, tmp_path, monkeypatch):
    from minimagen.Imagen import Imagen
    from minimagen.Unet import Unet, BaseTest, SuperTest
    from minimagen.t5 import get_encoded_dim
    from minimagen.training import (get_minimagen_parser, get_minimagen_dl_opts, create_directory, get_model_size, save_training_info,
                                    get_default_args, MinimagenTrain, load_testing_parameters, SyntheticCaptions)
    from minimagen_amd import optim, train_ops
    dev = setup(backend)
    monkeypatch.chdir(tmp_path)
    args = load_testing_parameters(get_minimagen_parser().parse_args(["-test", "-cn", "2"]))
    args.IMG_SIDE_LEN = 32
    args.EPOCHS = 1
    data = SyntheticCaptions(6, args.IMG_SIDE_LEN, get_encoded_dim(args.T5_NAME), max_words=args.MAX_NUM_WORDS, seed=1)
    train_ds, valid_ds = torch.utils.data.random_split(data, [4, 2], generator=torch.Generator().manual_seed(0))
    dl_opts = {**get_minimagen_dl_opts(dev), "batch_size": args.BATCH_SIZE, "num_workers": args.NUM_WORKERS}
    train_dl, valid_dl = torch.utils.data.DataLoader(train_ds, **dl_opts), torch.utils.data.DataLoader(valid_ds, **dl_opts)
    imagen_params = dict(image_sizes=(args.IMG_SIDE_LEN // 2, args.IMG_SIDE_LEN), timesteps=args.TIMESTEPS, cond_drop_prob=0.15, text_encoder_name=args.T5_NAME)

    def run(stamp, **kw):
        training_dir = create_directory(f"./training_{stamp}")
        unets_params = [get_default_args(BaseTest), get_default_args(SuperTest)]
        torch.manual_seed(0)
        unets = [Unet(**p).to(dev) for p in unets_params]
        imagen = Imagen(unets=unets, **imagen_params).to(dev)
        save_training_info(args, stamp, [{**get_default_args(Unet), **p} for p in unets_params], {**get_default_args(Imagen), **imagen_params},
                           get_model_size(imagen), training_dir)
        before = [p.detach().clone() for p in imagen.parameters()]
        optimizer = optim.Adam(imagen.parameters(), lr=args.OPTIM_LR)
        train_ops.FORCE = backend == "emu"
        try:
            MinimagenTrain(stamp, args, unets, imagen, train_dl, valid_dl, training_dir, optimizer, timeout=600, fail_fast=True, **kw)
        finally:
            train_ops.FORCE = False
        return imagen, before

    def listing(stamp):
        root = tmp_path / f"training_{stamp}"
        return sorted(os.path.relpath(os.path.join(d, f), root).replace(stamp, "<ts>") for d, _, fs in os.walk(root) for f in fs)
    with pytest.raises(ValueError, match="grad_clip"):
        run("20260101_000009", grad_clip="triton")
    run("20260101_000000")                                       # the default, for its files
    calls = []

    def no_torch_clip(*a, **k):
        calls.append(1)
        raise RuntimeError("torch.nn.utils.clip_grad_norm_ was called")
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", no_torch_clip)
    imagen, before = run("20260101_000001", grad_clip="device")
    assert not calls
    text = (tmp_path / "training_20260101_000001" / "training_progess.txt").read_text()
    assert "TRAINING ABORTED" not in text and text.count("Checkpoint created at batch number") >= 1
    assert listing("20260101_000001") == listing("20260101_000000") and any(f.startswith("state_dicts") for f in listing("20260101_000001"))
    after = list(imagen.parameters())
    assert all(bool(torch.isfinite(p).all()) for p in after) and sum(not same_bits(p, b) for p, b in zip(after, before)) > len(after) // 2
    with pytest.raises(RuntimeError, match="clip_grad_norm_ was called"):      # the default still goes where it went
        run("20260101_000002")
    assert calls
