"""Exponential moving average of the weights: the three kernels (mi_ema_update, mi_adam_ema_step, mi_ema_swap), ``optim.EMA`` with
and without an attached ``optim.Adam``, sampling and training around ``average_parameters()``, and the training loop's files."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from minimagen_amd import _lib as L
from oracle import restated as R
from tests._backend import BACKENDS, setup

SHAPES = [(1,), (16,), (255,), (256,), (257,), (4096,), (4097,), (5000,), (33, 129), (16, 8, 3, 3)]
TINY = dict(dim=8, dim_mults=(1, 2), num_resnet_blocks=1, layer_attns=False, layer_cross_attns=False, memory_efficient=True)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def spread(shape, gen):
    """fp32 values of either sign with magnitudes 2^-20 ... 2^10"""
    return (torch.rand(shape, generator=gen) * 2 - 1).sign() * torch.exp2(torch.rand(shape, generator=gen) * 30 - 20)


def ema_block(es, ps, w, dev):
    """(mi_ema_params, tensors to keep alive) over the pairs (es[k], ps[k])"""
    from minimagen_amd.optim import CHUNK, _upload
    rows = [(e.data_ptr(), p.data_ptr(), p.numel()) for e, p in zip(es, ps)]
    tens, ct, co, n = _upload(rows, dev)
    a = L.MiEmaParams()
    a.tensors, a.chunk_tensor, a.chunk_off, a.nchunks, a.chunk, a.w = tens.data_ptr(), ct.data_ptr(), co.data_ptr(), n, CHUNK, w
    return a, (tens, ct, co)


def adam_block(ps, gs, ms, vs, dev, *, weight_decay, grad_scale, t=3):
    from minimagen_amd.optim import CHUNK, _upload
    rows = [(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()) for p, g, m, v in zip(ps, gs, ms, vs)]
    tens, ct, co, n = _upload(rows, dev)
    a = L.MiAdamParams()
    a.tensors, a.chunk_tensor, a.chunk_off, a.nchunks, a.chunk = tens.data_ptr(), ct.data_ptr(), co.data_ptr(), n, CHUNK
    a.lr, a.beta1, a.beta2, a.eps, a.weight_decay = 1e-2, 0.9, 0.999, 1e-8, weight_decay
    a.bias_correction1, a.bias_correction2, a.one_minus_beta1, a.one_minus_beta2 = 1.0 - 0.9 ** t, 1.0 - 0.999 ** t, 1.0 - 0.9, 1.0 - 0.999
    a.grad_scale = grad_scale.data_ptr() if grad_scale is not None else None
    return a, (tens, ct, co)


# ------------------------------------------------------------------------------------------------ 1. host only
def test_schedule_and_validation():
    from minimagen_amd.optim import EMA
    named = [("a", torch.nn.Parameter(torch.zeros(3)))]
    e = EMA(named, decay=0.9999)
    assert [e.decay_at(k) for k in range(1, 6)] == [2 / 11, 3 / 12, 4 / 13, 5 / 14, 6 / 15]
    assert e.decay_at(10 ** 6) == 0.9999 and e.decay_at(89990) == 0.9999 and e.decay_at(89980) < 0.9999
    assert [e.advance() for _ in range(3)] == [1.0 - 2 / 11, 1.0 - 3 / 12, 1.0 - 4 / 13] and (e.step, e.num_updates) == (3, 3)
    e = EMA(named, decay=0.5, warmup=False)
    assert [e.decay_at(k) for k in (1, 2, 1000)] == [0.5, 0.5, 0.5] and e.advance() == 0.5
    e = EMA(named, decay=0.2)                                   # warmup never exceeds the decay asked for
    assert e.decay_at(1) == 2 / 11 and e.decay_at(2) == 0.2 and e.decay_at(50) == 0.2
    # the first update_after_step optimiser steps copy; k starts counting after them
    e = EMA(named, decay=0.9999, update_after_step=3)
    assert [e.advance() for _ in range(5)] == [1.0, 1.0, 1.0, 1.0 - 2 / 11, 1.0 - 3 / 12] and e.num_updates == 2
    # only every m-th step updates
    e = EMA(named, decay=0.9999, update_every=3)
    assert [e.advance() for _ in range(7)] == [None, None, 1.0 - 2 / 11, None, None, 1.0 - 3 / 12, None] and (e.step, e.num_updates) == (7, 2)
    e = EMA(named, decay=0.9999, update_every=2, update_after_step=2)
    assert [e.advance() for _ in range(6)] == [None, 1.0, None, 1.0 - 2 / 11, None, 1.0 - 3 / 12]
    for kw in (dict(decay=1.0), dict(decay=-0.1), dict(decay=1.5), dict(decay=float("nan")), dict(update_after_step=-1), dict(update_every=0),
               dict(update_every=-2), dict(update_every=1.5), dict(update_after_step=0.5)):
        with pytest.raises(ValueError):
            EMA(named, **kw)
    with pytest.raises(ValueError):
        EMA([])
    with pytest.raises(ValueError):
        EMA(named + named)
    lin = torch.nn.Linear(3, 2)
    e = EMA(lin)
    assert e.names == ["weight", "bias"] and all(s.dtype == torch.float32 and s.data_ptr() != p.data_ptr() and torch.equal(s, p.detach())
                                                  for s, p in zip(e.shadows, e.params))
    with pytest.raises(TypeError):
        e.attach(torch.optim.Adam(lin.parameters()))


# ------------------------------------------------------------------------------------------------ 2 - 4. kernels
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("w", [1e-4, 0.3, 1.0])
def test_ema_update_against_fp64(backend, w):
    """e <- fmaf(p - e, w, e): one rounding of p - e and one of the fma, each 2^-24 relative -> |e - e64| <= 2^-22 max(|p|, |e_old|);
    w = 1 is the exact copy"""
    dev = setup(backend)
    g = torch.Generator().manual_seed(5)
    p0, e0 = [spread(s, g) for s in SHAPES], [spread(s, g) for s in SHAPES]
    ps, es = [t.clone().to(dev) for t in p0], [t.clone().to(dev) for t in e0]
    a, keep = ema_block(es, ps, w, dev)
    L.check(L.lib().mi_ema_update(C.byref(a), L.current_stream()), "mi_ema_update")
    w32 = float(np.float32(w))
    worst = 0.0
    for p, e, pn, en in zip(p0, e0, ps, es):
        assert same_bits(pn, p)                                  # the parameter is only read
        ref = e.double() + (p.double() - e.double()) * w32
        err = (en.cpu().double() - ref).abs()
        bound = 2.0 ** -22 * torch.maximum(p.abs(), e.abs()).double()
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (tuple(p.shape), float((err / bound).max()))
        if w == 1.0:
            assert same_bits(en, p)
    print(f"mi_ema_update w={w}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("backend", BACKENDS)
def test_ema_entries_reject_bad_blocks(backend):
    dev = setup(backend)
    lib = L.lib()
    p, e = torch.ones(8, device=dev), torch.zeros(8, device=dev)
    good, keep = ema_block([e], [p], 0.5, dev)
    ad, keep2 = adam_block([p], [torch.ones(8, device=dev)], [torch.zeros(8, device=dev)], [torch.zeros(8, device=dev)], dev, weight_decay=0., grad_scale=None)

    def variant(**kw):
        b = L.MiEmaParams.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(b, k, v)
        return b
    empties = [variant(nchunks=0), variant(chunk=0), variant(tensors=None), variant(chunk_tensor=None), variant(chunk_off=None)]
    for b in empties:
        for fn in (lib.mi_ema_update, lib.mi_ema_swap):
            assert fn(C.byref(b), L.current_stream()) == -1 and b"empty / missing tables" in lib.mi_last_error()
    assert lib.mi_ema_update(None, L.current_stream()) == -1 and lib.mi_ema_swap(None, L.current_stream()) == -1
    for w in (-0.1, 1.5, float("nan")):
        assert lib.mi_ema_update(C.byref(variant(w=w)), L.current_stream()) == -1 and b"[0, 1]" in lib.mi_last_error()
        assert lib.mi_adam_ema_step(C.byref(ad), C.byref(variant(w=w)), L.current_stream()) == -1 and b"[0, 1]" in lib.mi_last_error()
    assert lib.mi_adam_ema_step(C.byref(ad), None, L.current_stream()) == -1 and b"empty / missing tables" in lib.mi_last_error()
    assert lib.mi_adam_ema_step(C.byref(ad), C.byref(variant(tensors=None)), L.current_stream()) == -1
    assert lib.mi_adam_ema_step(None, C.byref(good), L.current_stream()) == -1
    bad_adam = L.MiAdamParams.from_buffer_copy(ad)
    bad_adam.nchunks = 0
    assert lib.mi_adam_ema_step(C.byref(bad_adam), C.byref(good), L.current_stream()) == -1 and b"empty / missing tables" in lib.mi_last_error()
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert torch.equal(p.cpu(), torch.ones(8)) and torch.equal(e.cpu(), torch.zeros(8))        # nothing was launched


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
@pytest.mark.parametrize("scaled", [False, True])
def test_fused_equals_adam_then_update(backend, weight_decay, scaled):
    """mi_adam_ema_step leaves the bits of mi_adam_step followed by mi_ema_update in p, m, v and e"""
    dev = setup(backend)
    lib = L.lib()
    g = torch.Generator().manual_seed(9)
    host = dict(p=[torch.randn(s, generator=g) for s in SHAPES], g=[torch.randn(s, generator=g) * 10.0 ** (k % 5 - 3) for k, s in enumerate(SHAPES)],
                m=[torch.randn(s, generator=g) * 0.1 for s in SHAPES], v=[torch.rand(s, generator=g) * 0.01 for s in SHAPES],
                e=[torch.randn(s, generator=g) for s in SHAPES])
    scale = torch.tensor([0.5], device=dev) if scaled else None
    for w in (0.25, 1.0):
        two = {k: [t.clone().to(dev) for t in v] for k, v in host.items()}
        one = {k: [t.clone().to(dev) for t in v] for k, v in host.items()}
        a2, k2 = adam_block(two["p"], two["g"], two["m"], two["v"], dev, weight_decay=weight_decay, grad_scale=scale)
        e2, k2e = ema_block(two["e"], two["p"], w, dev)
        L.check(lib.mi_adam_step(C.byref(a2), L.current_stream()), "mi_adam_step")
        L.check(lib.mi_ema_update(C.byref(e2), L.current_stream()), "mi_ema_update")
        a1, k1 = adam_block(one["p"], one["g"], one["m"], one["v"], dev, weight_decay=weight_decay, grad_scale=scale)
        e1, k1e = ema_block(one["e"], one["p"], w, dev)
        e1.chunk_tensor = e1.chunk_off = None                    # the fused entry reads the shadows' table only
        e1.nchunks = 0
        L.check(lib.mi_adam_ema_step(C.byref(a1), C.byref(e1), L.current_stream()), "mi_adam_ema_step")
        for name in "pmve":
            for s, x, y in zip(SHAPES, one[name], two[name]):
                assert same_bits(x, y), (name, s, w)
        for x, y in zip(one["g"], host["g"]):
            assert same_bits(x, y)
        assert not same_bits(one["p"][7], host["p"][7]) and not same_bits(one["e"][7], host["e"][7])
        if w == 1.0:
            assert all(same_bits(x, y) for x, y in zip(one["e"], one["p"]))
    if scaled:                                                   # the device scalar is in effect: a different result without it
        plain = {k: [t.clone().to(dev) for t in v] for k, v in host.items()}
        a0, k0 = adam_block(plain["p"], plain["g"], plain["m"], plain["v"], dev, weight_decay=weight_decay, grad_scale=None)
        e0, k0e = ema_block(plain["e"], plain["p"], 1.0, dev)
        L.check(lib.mi_adam_ema_step(C.byref(a0), C.byref(e0), L.current_stream()), "mi_adam_ema_step")
        assert not same_bits(plain["m"][7], one["m"][7])


@pytest.mark.parametrize("backend", BACKENDS)
def test_ema_swap_is_a_bit_copy(backend):
    dev = setup(backend)
    lib = L.lib()
    g = torch.Generator().manual_seed(2)
    special = torch.tensor([0x7FC12345, 0xFFA00001 - (1 << 32), 0x80000000 - (1 << 32), 0x7F800000, 0xFF800000 - (1 << 32), 0x00000001,
                            0x807FFFFF - (1 << 32), 0x00400000, 0, 0x3F800000], dtype=torch.int32)
    p0, e0 = [], []
    for s in SHAPES:
        a, b = spread(s, g).reshape(-1), spread(s, g).reshape(-1)
        n = min(a.numel(), special.numel())
        a.view(torch.int32)[-n:] = special[:n]
        b.view(torch.int32)[:n] = special.flip(0)[:n]
        p0.append(a.reshape(s)), e0.append(b.reshape(s))
    ps, es = [t.clone().to(dev) for t in p0], [t.clone().to(dev) for t in e0]
    a, keep = ema_block(es, ps, 0.0, dev)
    L.check(lib.mi_ema_swap(C.byref(a), L.current_stream()), "mi_ema_swap")
    for p, e, pn, en in zip(p0, e0, ps, es):
        assert same_bits(pn, e) and same_bits(en, p), tuple(p.shape)
    L.check(lib.mi_ema_swap(C.byref(a), L.current_stream()), "mi_ema_swap")
    for p, e, pn, en in zip(p0, e0, ps, es):
        assert same_bits(pn, p) and same_bits(en, e), tuple(p.shape)


# ------------------------------------------------------------------------------------------------ 5, 6. EMA + Adam
ADAM_SHAPES = [(16, 8, 3, 3), (16,), (5000,), (3, 7), (1,), (33, 129), (7, 5)]          # the last one is float64: Adam's slow path


def _adam_setup(dev, g):
    base = [torch.randn(s, generator=g) for s in ADAM_SHAPES]
    base[-1] = base[-1].double()
    mine = [torch.nn.Parameter(b.clone().to(dev)) for b in base]
    ref = [torch.nn.Parameter(b.clone()) for b in base]
    groups = lambda ps: [dict(params=ps[:4]), dict(params=ps[4:], weight_decay=0.01, lr=3e-3)]
    return mine, ref, groups


def _grads(step, mine, ref, g, dev):
    for k, (a, b) in enumerate(zip(mine, ref)):
        if k == 3 and step % 2:                                  # no gradient on odd steps: its own step count, and no Adam launch row
            a.grad = b.grad = None
            continue
        gr = (torch.randn(a.shape, generator=g) * (10.0 ** (k % 6 - 3))).to(b.dtype)
        a.grad, b.grad = gr.clone().to(dev), gr.clone()


@pytest.mark.parametrize("backend", BACKENDS)
def test_ema_with_adam_matches_reference(backend):
    """6 steps of Adam with an attached EMA against torch.optim.Adam and an fp64 running average of ITS parameters.  Gates: parameters at
    test_adam_kernel_matches_torch_adam's 2e-6 max(1, max|ref|); shadows at 4e-6 max(1, max|ref|) -- the parameter gate carried through a
    convex combination, plus at most six fp32 roundings (2^-24 relative each)"""
    from minimagen_amd.optim import Adam, EMA
    dev = setup(backend)
    g = torch.Generator().manual_seed(3)
    mine, ref, groups = _adam_setup(dev, g)
    plain = [torch.nn.Parameter(p.detach().clone()) for p in mine]           # an optimiser with nothing attached
    om, op, orf = Adam(groups(mine), lr=1e-2), Adam(groups(plain), lr=1e-2), torch.optim.Adam(groups(ref), lr=1e-2, foreach=False)
    ema = EMA([(f"p{k}", p) for k, p in enumerate(mine)], decay=0.9).attach(om)
    avg = [b.detach().double().clone() for b in ref]
    for step in range(6):
        _grads(step, mine, ref, g, dev)
        for a, b in zip(plain, mine):
            b_grad = b.grad
            a.grad = None if b_grad is None else b_grad.clone()
        om.step(); op.step(); orf.step()
        d = min(0.9, (2.0 + step) / (11.0 + step))
        for s, b in zip(avg, ref):
            s.add_((b.detach().double() - s) * (1.0 - d))
    assert (ema.step, ema.num_updates) == (6, 6)
    for a, b, c in zip(mine, ref, plain):
        assert (a.detach().cpu() - b.detach()).abs().max() < 2e-6 * max(1.0, float(b.abs().max())), tuple(a.shape)
        assert torch.equal(a.detach().cpu(), c.detach().cpu())                # attaching changes no parameter bit
    for e, s, a in zip(ema.shadows, avg, mine):
        assert e.dtype == torch.float32 and e.device == a.device
        err = float((e.cpu().double() - s).abs().max())
        assert err < 4e-6 * max(1.0, float(s.abs().max())), (tuple(e.shape), err)
    # update() after the step of an optimiser with nothing attached: the same shadows, bit for bit, as the fused launch gave
    g2 = torch.Generator().manual_seed(3)
    mine2, ref2, groups2 = _adam_setup(dev, g2)
    o2 = Adam(groups2(mine2), lr=1e-2)
    ema2 = EMA([(f"p{k}", p) for k, p in enumerate(mine2)], decay=0.9)
    for step in range(6):
        _grads(step, mine2, ref2, g2, dev)
        o2.step(); ema2.update()
    assert all(same_bits(x, y) for x, y in zip(mine, mine2)) and all(same_bits(x, y) for x, y in zip(ema.shadows, ema2.shadows))


@pytest.mark.parametrize("backend", BACKENDS)
def test_update_every_and_update_after_step(backend):
    """update_every=2, update_after_step=2: step 1 stays put, step 2 copies, step 3 stays put, step 4 averages (k = 1), ..."""
    from minimagen_amd.optim import Adam, EMA
    dev = setup(backend)
    g = torch.Generator().manual_seed(3)
    mine, ref, groups = _adam_setup(dev, g)
    om = Adam(groups(mine), lr=1e-2)
    ema = EMA([(f"p{k}", p) for k, p in enumerate(mine)], decay=0.9, update_every=2, update_after_step=2).attach(om)
    start = [p.detach().clone() for p in mine]
    for step in range(1, 5):
        before = [e.clone() for e in ema.shadows]
        _grads(step - 1, mine, ref, g, dev)
        om.step()
        for k, (e, old, p) in enumerate(zip(ema.shadows, before, mine)):
            if step in (1, 3):
                assert same_bits(e, old), (step, k)
            elif step == 2:
                assert same_bits(e, p.detach().float()) and (k == 3 or not same_bits(e, start[k].float())), (step, k)
            else:
                want = old.cpu().double() + (p.detach().cpu().double() - old.cpu().double()) * (1.0 - 2 / 11)
                assert not same_bits(e, old) and (e.cpu().double() - want).abs().max() <= 2.0 ** -22 * max(float(p.abs().max()), float(old.abs().max()))
    assert (ema.step, ema.num_updates) == (4, 1)


@pytest.mark.parametrize("backend", BACKENDS)
def test_state_dict_round_trip(backend, tmp_path):
    from minimagen_amd.optim import Adam, EMA
    dev = setup(backend)
    g = torch.Generator().manual_seed(3)
    mine, ref, groups = _adam_setup(dev, g)
    om = Adam(groups(mine), lr=1e-2)
    names = [f"p{k}" for k in range(len(mine))]
    ema = EMA(zip(names, mine), decay=0.95, update_every=1, update_after_step=1).attach(om)
    for step in range(3):
        _grads(step, mine, ref, g, dev)
        om.step()
    torch.save(dict(ema=ema.state_dict(), opt=om.state_dict(), params=[p.detach().clone() for p in mine]), tmp_path / "s.pth")
    saved = torch.load(tmp_path / "s.pth", map_location=dev)
    assert saved["ema"]["step"] == 3 and saved["ema"]["num_updates"] == 2 and set(saved["ema"]["shadows"]) == set(names)
    fresh = [torch.nn.Parameter(p.clone()) for p in saved["params"]]
    of = Adam(groups(fresh), lr=1e-2)
    of.load_state_dict(saved["opt"])
    ema_f = EMA(zip(names, fresh), decay=0.5, warmup=False).attach(of)        # other hyper-parameters: the loaded state wins
    ema_f.load_state_dict(saved["ema"])
    assert (ema_f.decay, ema_f.warmup, ema_f.update_after_step, ema_f.step, ema_f.num_updates) == (0.95, True, 1, 3, 2)
    for step in range(3, 6):
        _grads(step, mine, ref, g, dev)
        for a, b in zip(fresh, mine):
            a.grad = None if b.grad is None else b.grad.clone()
        om.step(); of.step()
    assert all(same_bits(x, y) for x, y in zip(mine, fresh))
    assert all(same_bits(x, y) for x, y in zip(ema.shadows, ema_f.shadows))
    with pytest.raises(KeyError):
        ema_f.load_state_dict({**saved["ema"], "shadows": {"other": torch.zeros(1)}})
    # copy_to: the averages into a second model's parameters, by name
    class Holder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            for n, p in zip(names, mine):
                self.register_parameter(n, torch.nn.Parameter(torch.zeros_like(p)))
    h = Holder()
    ema.copy_to(h)
    assert all(torch.equal(getattr(h, n).detach().cpu(), e.cpu().to(getattr(h, n).dtype)) for n, e in zip(names, ema.shadows))


@pytest.mark.parametrize("backend", BACKENDS)
def test_inside_average_parameters_the_state_is_the_averages(backend):
    """inside average_parameters() the shadows' buffers hold the live weights: state_dict() and copy_to() still give the averages, bit for
    bit what they give outside, and everything that would update or overwrite the shadows raises without moving a counter or a bit"""
    from minimagen_amd.optim import Adam, EMA
    dev = setup(backend)
    g = torch.Generator().manual_seed(3)
    mine, ref, groups = _adam_setup(dev, g)                      # (the float64 one is not exchanged by the kernel: stashed and restored)
    om = Adam(groups(mine), lr=1e-2)
    names = [f"p{k}" for k in range(len(mine))]
    ema = EMA(zip(names, mine), decay=0.9).attach(om)
    for step in range(3):
        _grads(step, mine, ref, g, dev)
        om.step()
    _grads(3, mine, ref, g, dev)
    outside = ema.state_dict()
    live = [p.detach().clone() for p in mine]
    assert all(not torch.equal(outside["shadows"][n].cpu().double(), p.cpu().double()) for n, p in zip(names, live))

    class Holder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            for n, p in zip(names, mine):
                self.register_parameter(n, torch.nn.Parameter(torch.zeros_like(p)))
    with ema.average_parameters():
        inside = ema.state_dict()
        h = Holder()
        ema.copy_to(h)
        for call in (ema.update, ema.advance, om.step, lambda: ema.load_state_dict(outside)):
            with pytest.raises(RuntimeError, match="inside average_parameters"):
                call()
        with pytest.raises(RuntimeError, match="does not nest"):
            with ema.average_parameters():
                pass
        again = ema.state_dict()
        assert all(same_bits(p, outside["shadows"][n].to(p.dtype)) for n, p in zip(names, mine))      # the parameters are the averages
    after = ema.state_dict()
    for d in (inside, again, after):
        assert {k: v for k, v in d.items() if k != "shadows"} == {k: v for k, v in outside.items() if k != "shadows"} and d["step"] == 3
        assert list(d["shadows"]) == names and all(same_bits(d["shadows"][n], outside["shadows"][n]) for n in names)
    assert all(same_bits(getattr(h, n), outside["shadows"][n].to(getattr(h, n).dtype)) for n in names)
    assert all(same_bits(p, k) for p, k in zip(mine, live)) and all(om._count[p] == (2 if k == 3 else 3) for k, p in enumerate(mine))
    om.step()                                                    # and outside the block everything works again
    assert (ema.step, ema.num_updates) == (4, 4) and not same_bits(ema.shadows[0], outside["shadows"]["p0"])


# ------------------------------------------------------------------------------------------------ 7. sampling from the averages
def _tiny_cascade(dev, seed=4):
    from minimagen_amd.Imagen import Imagen
    from minimagen_amd.Unet import Unet
    torch.manual_seed(seed)
    im = Imagen([Unet(**TINY), Unet(**TINY, lowres_cond=True)], text_encoder_name="t5_small", image_sizes=[16, 32], timesteps=25, cond_drop_prob=0.15)
    return im.to(dev)


@pytest.mark.parametrize("backend", BACKENDS)
def test_sampling_from_the_averages(backend):
    from minimagen_amd.optim import EMA
    dev = setup(backend)
    im = _tiny_cascade(dev)
    ema = EMA(im, decay=0.9)
    g = torch.Generator().manual_seed(8)
    with torch.no_grad():                                        # shadows that differ from the weights: updates against perturbed parameters
        keep = [p.detach().clone() for p in im.parameters()]
        for _ in range(3):
            for p, k in zip(im.parameters(), keep):
                p.copy_(k + 0.05 * torch.randn(k.shape, generator=g).to(dev))
            ema.update()
        for p, k in zip(im.parameters(), keep):
            p.copy_(k)
    emb, mask = R.synthetic_text(2, length=8, seed=1)
    kw = dict(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., _seed=11)
    before = im.sample(**kw).clone()
    versions = [p._version for p in im.parameters()]
    shadows = [e.clone() for e in ema.shadows]
    with ema.average_parameters():
        for p, e, k, v in zip(im.parameters(), shadows, keep, versions):
            assert same_bits(p, e) and p._version > v                          # (a)
        assert all(same_bits(e, k) for e, k in zip(ema.shadows, keep))
        inside = im.sample(**kw).clone()
        sds = [{k: v.detach().clone() for k, v in u.state_dict().items()} for u in im.unets]
    versions2 = [p._version for p in im.parameters()]
    assert all(same_bits(p, k) for p, k in zip(im.parameters(), keep)) and all(b > a for a, b in zip(versions, versions2))
    assert all(same_bits(e, s) for e, s in zip(ema.shadows, shadows))
    after = im.sample(**kw).clone()
    assert torch.equal(after, before)                                          # (c)
    assert not torch.equal(inside, before) and inside.isfinite().all()
    fresh = _tiny_cascade(dev, seed=99)
    for u, sd in zip(fresh.unets, sds):
        u.load_state_dict(sd)
    assert torch.equal(fresh.sample(**kw), inside)                             # (b)
    im.check_device_status()


# ------------------------------------------------------------------------------------------------ 8. training continuity
@pytest.mark.parametrize("backend", BACKENDS)
def test_training_continues_after_average_parameters(backend):
    """two training steps with an enter / exit of average_parameters() (and a forward on the averages) between them leave the bits of two
    steps without it: no weight pack or scale cache keeps the swapped-in values"""
    from minimagen_amd import train_ops
    from minimagen_amd.Imagen import Imagen
    from minimagen_amd.Unet import Unet
    from minimagen_amd.optim import Adam, EMA
    dev = setup(backend)
    emb, mask = R.synthetic_text(2, length=8, seed=1)
    emb, mask = emb.to(dev), mask.to(dev)
    images = torch.rand(2, 3, 16, 16, generator=torch.Generator().manual_seed(6)).to(dev)
    train_ops.FORCE = backend == "emu"
    try:
        results = []
        for visit in (False, True):
            torch.manual_seed(4)
            im = Imagen([Unet(**TINY)], text_encoder_name="t5_small", image_sizes=[16], timesteps=25, cond_drop_prob=0.15).to(dev)
            opt = Adam(im.parameters(), lr=1e-2)
            ema = EMA(im, decay=0.5, warmup=False).attach(opt)
            for step in range(2):
                torch.manual_seed(100 + step)
                im.train(True)
                loss = im(images, text_embeds=emb, text_masks=mask, unet_number=1)
                loss.backward()
                opt.step(); opt.zero_grad()
                if visit and step == 0:
                    live = [p.detach().clone() for p in im.parameters()]
                    with ema.average_parameters():
                        assert any(not same_bits(p, k) for p, k in zip(im.parameters(), live))
                        im.train(False)
                        with torch.no_grad():
                            torch.manual_seed(7)
                            assert torch.isfinite(im(images, text_embeds=emb, text_masks=mask, unet_number=1))
                    assert all(same_bits(p, k) for p, k in zip(im.parameters(), live))
            results.append(([p.detach().clone() for p in im.parameters()], [e.clone() for e in ema.shadows], float(loss)))
    finally:
        train_ops.FORCE = False
    (p0, e0, l0), (p1, e1, l1) = results
    assert l0 == l1 and all(same_bits(a, b) for a, b in zip(p0, p1)) and all(same_bits(a, b) for a, b in zip(e0, e1))


# ------------------------------------------------------------------------------------------------ 9. the loop and the directory
@pytest.mark.parametrize("backend", BACKENDS)
def test_train_flow_with_ema(backend, tmp_path, monkeypatch):
    from minimagen.Imagen import Imagen
    from minimagen.Unet import Unet, BaseTest, SuperTest
    from minimagen.generate import load_minimagen
    from minimagen.t5 import get_encoded_dim
    from minimagen.training import (get_minimagen_parser, get_minimagen_dl_opts, create_directory, get_model_size, save_training_info,
                                    get_default_args, MinimagenTrain, load_testing_parameters, SyntheticCaptions)
    from minimagen_amd import optim, train_ops
    dev = setup(backend)
    monkeypatch.chdir(tmp_path)
    args = load_testing_parameters(get_minimagen_parser().parse_args(["-test", "-cn", "2"]))
    args.IMG_SIDE_LEN = 32
    ts = "20260101_000000"
    data = SyntheticCaptions(8, args.IMG_SIDE_LEN, get_encoded_dim(args.T5_NAME), max_words=args.MAX_NUM_WORDS, seed=1)
    train_ds, valid_ds = torch.utils.data.random_split(data, [6, 2], generator=torch.Generator().manual_seed(0))
    dl_opts = {**get_minimagen_dl_opts(dev), "batch_size": args.BATCH_SIZE, "num_workers": args.NUM_WORKERS}
    train_dl, valid_dl = torch.utils.data.DataLoader(train_ds, **dl_opts), torch.utils.data.DataLoader(valid_ds, **dl_opts)
    imagen_params = dict(image_sizes=(args.IMG_SIDE_LEN // 2, args.IMG_SIDE_LEN), timesteps=args.TIMESTEPS, cond_drop_prob=0.15, text_encoder_name=args.T5_NAME)
    roots = {}
    for which in ("ema", "plain"):
        stamp = ts if which == "ema" else "20260101_000001"
        training_dir = create_directory(f"./training_{stamp}")
        unets_params = [get_default_args(BaseTest), get_default_args(SuperTest)]
        torch.manual_seed(0)
        unets = [Unet(**p).to(dev) for p in unets_params]
        imagen = Imagen(unets=unets, **imagen_params).to(dev)
        save_training_info(args, stamp, [{**get_default_args(Unet), **p} for p in unets_params], {**get_default_args(Imagen), **imagen_params},
                           get_model_size(imagen), training_dir)
        optimizer = optim.Adam(imagen.parameters(), lr=args.OPTIM_LR)
        ema = optim.EMA(imagen, decay=0.9) if which == "ema" else None
        if which == "plain":
            args.EPOCHS = 1                                      # (enough for a directory without EMA files)
        train_ops.FORCE = backend == "emu"
        try:
            MinimagenTrain(stamp, args, unets, imagen, train_dl, valid_dl, training_dir, optimizer, timeout=600, fail_fast=True, ema=ema)
        finally:
            train_ops.FORCE = False
        roots[which] = tmp_path / f"training_{stamp}"
    root = roots["ema"]
    assert optimizer._ema is None                                # (the run without an EMA: nothing attached)
    text = (root / "training_progess.txt").read_text()
    assert "TRAINING ABORTED" not in text and text.count("Checkpoint created at batch number") == 4
    assert text.count("U-Nets Avg Valid Losses: ") == 4 and text.count("U-Nets Best Valid Losses: ") == 4
    assert text.count("U-Nets Avg Valid Losses (EMA): ") == 4 and text.count("U-Nets Best Valid Losses (EMA): ") == 4
    assert sorted(os.listdir(root / "tmp")) == ["unet_0_tmp.pth", "unet_1_tmp.pth"]
    assert sorted(os.listdir(root / "state_dicts")) == [f"unet_0_state_{ts}.pth", f"unet_1_state_{ts}.pth"]
    assert sorted(os.listdir(root / "ema_tmp")) == ["ema_state.pth", "unet_0_tmp.pth", "unet_1_tmp.pth"]
    assert sorted(os.listdir(root / "ema_state_dicts")) == [f"unet_0_state_{ts}.pth", f"unet_1_state_{ts}.pth"]
    state = torch.load(root / "ema_tmp" / "ema_state.pth", map_location="cpu")
    assert state["decay"] == 0.9 and state["step"] == state["num_updates"] > 0 and all(k.startswith("unets.") for k in state["shadows"])
    # the EMA's own state holds the AVERAGES of that checkpoint -- the parameters of ema_tmp/unet_<i>_tmp.pth, not those of tmp/unet_<i>_tmp.pth
    for i in range(2):
        avg_i = torch.load(root / "ema_tmp" / f"unet_{i}_tmp.pth", map_location="cpu")
        raw_i = torch.load(root / "tmp" / f"unet_{i}_tmp.pth", map_location="cpu")
        mine_i = {k[len(f"unets.{i}."):]: v for k, v in state["shadows"].items() if k.startswith(f"unets.{i}.")}
        assert mine_i and set(mine_i) <= set(avg_i) and all(same_bits(v, avg_i[k]) for k, v in mine_i.items())
        assert sum(not same_bits(v, raw_i[k]) for k, v in mine_i.items()) > len(mine_i) // 2
    assert sum(len([k for k in state["shadows"] if k.startswith(f"unets.{i}.")]) for i in range(2)) == len(state["shadows"])
    averaged, raw = load_minimagen(str(root), ema=True), load_minimagen(str(root))
    differ = 0
    for k in range(2):
        on_disk_ema = torch.load(root / "ema_state_dicts" / f"unet_{k}_state_{ts}.pth", map_location="cpu")
        on_disk_raw = torch.load(root / "state_dicts" / f"unet_{k}_state_{ts}.pth", map_location="cpu")
        sd_a, sd_r = averaged.unets[k].state_dict(), raw.unets[k].state_dict()
        assert set(sd_a) == set(on_disk_ema) == set(on_disk_raw)
        assert all(torch.equal(v.cpu(), on_disk_ema[n]) for n, v in sd_a.items()) and all(torch.equal(v.cpu(), on_disk_raw[n]) for n, v in sd_r.items())
        assert all(torch.isfinite(v).all() for v in on_disk_ema.values())
        differ += sum(not torch.equal(on_disk_ema[n], on_disk_raw[n]) for n in on_disk_ema)
    assert differ > 0
    # the rolling files alone serve too
    for f in os.listdir(root / "ema_state_dicts"):
        os.remove(root / "ema_state_dicts" / f)
    rolling = load_minimagen(str(root), ema=True)
    tmp0 = torch.load(root / "ema_tmp" / "unet_0_tmp.pth", map_location="cpu")
    assert all(torch.equal(v.cpu(), tmp0[n]) for n, v in rolling.unets[0].state_dict().items())
    # a directory written without an EMA: today's files, and ema=True is an error
    plain = roots["plain"]
    assert sorted(os.listdir(plain)) == ["parameters", "state_dicts", "tmp", "training_progess.txt"] and "(EMA)" not in (plain / "training_progess.txt").read_text()
    with pytest.raises(ValueError):
        load_minimagen(str(plain), ema=True)
    load_minimagen(str(plain))


# ------------------------------------------------------------------------------------------------ 10. ABI
@pytest.mark.parametrize("backend", BACKENDS)
def test_abi_is_additive(backend):
    setup(backend)
    lib = L.lib()
    assert lib.mi_abi_version() == 12
    assert lib.mi_struct_size(28) == C.sizeof(L.MiEmaTensor) == 24 and lib.mi_struct_size(29) == C.sizeof(L.MiEmaParams) == 40
    assert lib.mi_struct_size(20) == C.sizeof(L.MiAdamTensor) == 40 and lib.mi_struct_size(21) == C.sizeof(L.MiAdamParams)
    assert lib.mi_struct_size(30) == -1
    for name in ("mi_ema_update", "mi_adam_ema_step", "mi_ema_swap"):
        getattr(lib, name)
