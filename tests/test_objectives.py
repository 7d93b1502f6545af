"""Prediction objectives ('noise' | 'x_start' | 'v') and the min-SNR-gamma loss weight: the coefficient and weight
tables (host, against an fp64 restatement from the betas written here), the constructor keywords, the torch-op form of the training loss,
the kernels of csrc/objective.hip (mi_diffuse_fwd bit for bit, the loss kernels against fp64), the training step on the device path, and
sampling against a restated loop on a table whose columns 0 and 1 are rebuilt here (the project's gate: max|d| < 1e-4, mean|d| < 1e-5)."""
import ctypes as C
import json
import os
import types

import pytest
import torch
import torch.nn.functional as F

from minimagen_amd import _lib as L
from minimagen_amd.Imagen import Imagen
from minimagen_amd.Unet import Unet
from minimagen_amd.diffusion_model import GaussianDiffusion
from oracle import restated as R
from tests import _inputs as I
from tests._backend import BACKENDS, GPU_ONLY, setup

OBJECTIVES = ("noise", "x_start", "v")
LOSS_TYPES = ("l1", "l2", "huber")
TINY = dict(dim=8, dim_mults=(1, 2), num_resnet_blocks=1, layer_attns=False, layer_cross_attns=False, memory_efficient=False)
BASE = dict(dim=8, dim_mults=(1, 2), num_resnet_blocks=1, layer_attns=False, layer_cross_attns=False, memory_efficient=False)
SR = dict(dim=8, dim_mults=(1, 2), num_resnet_blocks=(1, 2), layer_attns=False, layer_cross_attns=False, memory_efficient=True)


# ------------------------------------------------------------------------------------------------ the fp64 restatement (nothing from the code under test)
def abar64(T):
    betas = torch.linspace(1000 / T * 0.0001, 1000 / T * 0.02, T, dtype=torch.float64)
    return torch.cumprod(1. - betas, dim=0)


def columns64(a, objective):
    """columns 0 and 1 of a coefficient table whose rows sit at abar = a: x0 = c0 x_t - c1 pred"""
    if objective == "noise":
        return torch.stack(((1. / a).sqrt(), (1. / a - 1).sqrt()), dim=1)
    if objective == "v":
        return torch.stack((a.sqrt(), (1. - a).sqrt()), dim=1)
    return torch.stack((torch.zeros_like(a), -torch.ones_like(a)), dim=1)


def weights64(T, objective, gamma):
    a = abar64(T)
    out = []
    for ab in a.tolist():
        snr = ab / (1. - ab)
        c = min(snr, gamma)
        if objective == "noise":
            out.append(c / snr if snr > 0. else 1.)
        elif objective == "x_start":
            out.append(c)
        else:
            out.append(c / (snr + 1.))
    return torch.tensor(out, dtype=torch.float64)


def loss64(d, loss_type):
    if loss_type == "l1":
        return d.abs()
    if loss_type == "l2":
        return d * d
    return torch.where(d.abs() < 1., 0.5 * d * d, d.abs() - 0.5)


def slope64(d, loss_type):
    if loss_type == "l1":
        return d.sign()
    if loss_type == "l2":
        return 2. * d
    return torch.where(d.abs() < 1., d, d.sign())


def target64(objective, x0, eps, a, s):
    return {"noise": eps, "x_start": x0, "v": a * eps - s * x0}[objective]


# ------------------------------------------------------------------------------------------------ host, no backend
@pytest.mark.parametrize("T", [20, 100, 1000])
def test_coefficient_tables(T):
    gd = GaussianDiffusion(timesteps=T)
    a_all = abar64(T)
    assert torch.equal(gd.sampler_coef_table(), gd.sampler_coef_table(objective="noise"))
    assert torch.equal(gd.sampler_coef_table(known=True), gd.sampler_coef_table(known=True, objective="noise"))
    g = torch.Generator().manual_seed(T)
    x0, eps = torch.randn(T, 5, generator=g, dtype=torch.float64), torch.randn(T, 5, generator=g, dtype=torch.float64)
    # the default loop's table: fp32 only -- the restated columns rounded once, the other columns those of the 'noise' table
    base = gd.sampler_coef_table(known=True)
    for obj in ("v", "x_start"):
        tab = gd.sampler_coef_table(known=True, objective=obj)
        assert tab.dtype == torch.float32 and torch.equal(tab[:, :2], columns64(a_all, obj).to(torch.float32)) and torch.equal(tab[:, 2:], base[:, 2:])
        assert torch.equal(gd.sampler_coef_table(objective=obj)[:, :6], tab[:, :6])
    for sampler, eta in (("ddpm", None), ("ddim", None), ("ddim", 0.5), ("dpmpp_2m", None)):
        for S in (2, 7, T):
            tau0, tab0 = gd.sampler_tables(S, sampler, eta)
            tau1, tab1 = gd.sampler_tables(S, sampler, eta, objective="noise")
            assert torch.equal(tau0, tau1) and torch.equal(tab0, tab1)
            _, a, ref64 = gd._sampler_tables64(S, sampler, eta, True)
            assert torch.equal(a, a_all[tau0])
            for obj in ("v", "x_start"):
                tau, a2, t64 = gd._sampler_tables64(S, sampler, eta, True, obj)
                assert torch.equal(tau, tau0) and torch.equal(a2, a) and torch.equal(t64[:, 2:], ref64[:, 2:])          # columns 2-7: the solver's alone
                al, sg = a.sqrt()[:, None], (1. - a).sqrt()[:, None]
                xs, es = x0[:S], eps[:S]
                x_t = al * xs + sg * es
                pred = target64(obj, xs, es, al, sg)
                assert (t64[:, 0:1] * x_t - t64[:, 1:2] * pred - xs).abs().max() < 1e-12, (sampler, S, obj)
                t32 = gd.sampler_tables(S, sampler, eta, True, obj)[1]
                assert torch.equal(t32, t64.to(torch.float32)) and torch.equal(t32[:, :2], columns64(a, obj).to(torch.float32))
                if obj == "x_start":
                    assert (t32[:, 0] == 0).all() and (t32[:, 1] == -1).all() and (t64[:, 0] == 0).all() and (t64[:, 1] == -1).all()
    with pytest.raises(ValueError):
        gd.sampler_coef_table(objective="eps")
    with pytest.raises(ValueError):
        gd.sampler_tables(5, "ddim", None, False, "velocity")


@pytest.mark.parametrize("T", [20, 100, 1000])
def test_loss_weight_tables(T):
    gd = GaussianDiffusion(timesteps=T)
    if T == 20:
        assert abar64(T)[-1] == 0.                       # the case the limits are for
    for obj in OBJECTIVES:
        assert torch.equal(gd.loss_weight_table(obj), torch.ones(T)) and torch.equal(gd.loss_weight_table(obj, None), torch.ones(T))
        for gamma in (5., 1., 20.):
            w = gd.loss_weight_table(obj, gamma)
            ref = weights64(T, obj, gamma)
            assert w.dtype == torch.float32 and w.shape == (T,) and torch.isfinite(w).all()
            assert (w.double() - ref).abs().max() <= 2. ** -23 * ref.abs().max() and ((w.double() - ref).abs() <= 2. ** -23 * ref.abs() + 1e-300).all()
            assert (w >= 0).all() and (w <= (gamma if obj == "x_start" else 1.)).all()
            if T == 20:
                assert w[-1] == (1. if obj == "noise" else 0.)
        with pytest.raises(ValueError):
            gd.loss_weight_table(obj, 0.)
        with pytest.raises(ValueError):
            gd.loss_weight_table(obj, -1.)
    with pytest.raises(ValueError):
        gd.loss_weight_table("eps", 5.)


def test_tensor_helpers():
    gd = GaussianDiffusion(timesteps=100)
    g = torch.Generator().manual_seed(1)
    x0, eps = torch.randn(4, 3, 8, 8, generator=g), torch.randn(4, 3, 8, 8, generator=g)
    t = torch.tensor([0, 17, 60, 99])
    a, s = abar64(100)[t].sqrt().reshape(4, 1, 1, 1), (1 - abar64(100)[t]).sqrt().reshape(4, 1, 1, 1)
    v = gd.calculate_v(x0, t, eps)
    assert v.dtype == torch.float32 and (v.double() - (a * eps.double() - s * x0.double())).abs().max() < 1e-6
    back = gd.predict_start_from_v(gd.q_sample(x0, t, eps), t, v)
    assert (back - x0).abs().max() < 1e-5


def _two_unets():
    return [Unet(**TINY), Unet(**TINY, lowres_cond=True)]


def test_argument_validation():
    kw = dict(text_encoder_name="t5_small", image_sizes=(16, 32), timesteps=25)
    im = Imagen(_two_unets(), **kw)
    assert im.pred_objectives == ("noise", "noise") and im.min_snr_loss_weight == (False, False) and im.min_snr_gamma == (5., 5.)
    im = Imagen(_two_unets(), **kw, pred_objectives=["x_start", "v"], min_snr_loss_weight=[True, False], min_snr_gamma=[5, 2.5])      # lists: the parameter JSON's form
    assert im.pred_objectives == ("x_start", "v") and im.min_snr_loss_weight == (True, False) and im.min_snr_gamma == (5., 2.5)
    im = Imagen(_two_unets(), **kw, pred_objectives="v", min_snr_loss_weight=True, min_snr_gamma=3.)
    assert im.pred_objectives == ("v", "v") and im.min_snr_loss_weight == (True, True) and im.min_snr_gamma == (3., 3.)
    bad = [dict(pred_objectives="eps"), dict(pred_objectives=("v",)), dict(pred_objectives=("v", "v", "v")), dict(pred_objectives=("v", "velocity")),
           dict(pred_objectives=None), dict(min_snr_gamma=0.), dict(min_snr_gamma=-5.), dict(min_snr_gamma=(5., 0.)), dict(min_snr_gamma=(5.,)),
           dict(min_snr_gamma=float("nan")), dict(min_snr_loss_weight=(True,)), dict(min_snr_loss_weight=(True, False, True)), dict(min_snr_loss_weight="yes")]
    for b in bad:
        with pytest.raises(ValueError):
            Imagen(_two_unets(), **kw, **b)
    with pytest.raises(TypeError):
        Imagen(_two_unets(), "t5_small", (16, 32), None, 3, 25, 0.1, "l2", 0.2, True, 0.9, None, "v")          # keyword-only


def test_explicit_defaults_are_the_default_loss():
    emb, mask = R.synthetic_text(3, length=7, seed=2)
    imgs = torch.rand(3, 3, 40, 40)
    losses = []
    for extra in ({}, dict(pred_objectives="noise", min_snr_loss_weight=False, min_snr_gamma=5.), dict(pred_objectives=("noise", "noise"), min_snr_gamma=(2., 7.))):
        torch.manual_seed(1)
        im = Imagen((Unet(**BASE), Unet(**SR)), text_encoder_name="t5_small", image_sizes=(16, 32), timesteps=50, **extra).train()
        per = []
        for n in (1, 2):
            torch.manual_seed(9)
            per.append(im(imgs, text_embeds=emb, text_masks=mask, unet_number=n).detach())
        losses.append(per)
    for per in losses[1:]:
        assert torch.equal(per[0], losses[0][0]) and torch.equal(per[1], losses[0][1])


@pytest.mark.parametrize("loss_type", LOSS_TYPES)
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_torch_op_form_against_fp64(objective, loss_type):
    """Imagen._p_losses in torch ops (no backend) with the min-SNR weight against the fp64 restatement of the front and the loss: x_t, the target,
    the weight, the loss and dloss/dpred are formed here in fp64 from the betas; the U-Net itself (fp32 only: its time embedding is) maps the
    restated x_t to pred and carries the restated dloss/dpred back to its parameters.  The project's gates for a training step
    (tests/test_training.py: loss 1e-5 relative, gradients 1e-4 max(1e-3, max|g|))"""
    T, B, gamma = 50, 3, 5.
    torch.manual_seed(3)
    im = Imagen((Unet(**TINY),), text_encoder_name="t5_small", image_sizes=(16,), timesteps=T, cond_drop_prob=0., loss_type=loss_type,
                pred_objectives=objective, min_snr_loss_weight=True, min_snr_gamma=gamma).train()
    g = torch.Generator().manual_seed(4)
    x = torch.rand(B, 3, 16, 16, generator=g)
    eps = torch.randn(B, 3, 16, 16, generator=g)
    times = torch.tensor([0, T - 1, 23])
    emb, mask = R.synthetic_text(B, length=7, seed=2)
    loss = im._p_losses(im.unets[0], x, times, noise_scheduler=im.noise_schedulers[0], text_embeds=emb, text_mask=mask, noise=eps, unet_index=0)
    loss.backward()
    got = {n: p.grad.clone() for n, p in im.unets[0].named_parameters()}
    im.zero_grad(set_to_none=True)
    a = abar64(T)[times].sqrt().reshape(B, 1, 1, 1)
    s = (1. - abar64(T)[times]).sqrt().reshape(B, 1, 1, 1)
    x0 = x.double() * 2 - 1
    pred = im.unets[0](x_t := (a * x0 + s * eps.double()).float(), times, text_embeds=emb, text_mask=mask, cond_drop_prob=0.)
    d = pred.detach().double() - target64(objective, x0, eps.double(), a, s)
    w = weights64(T, objective, gamma)[times]
    ref = float((w * loss64(d, loss_type).flatten(1).sum(dim=1)).sum() / (B * 3 * 16 * 16))
    pred.backward((w.reshape(B, 1, 1, 1) * slope64(d, loss_type) / (B * 3 * 16 * 16)).float())
    print(f"{objective} {loss_type}: loss {loss.item():.7f} vs fp64 {ref:.7f}")
    assert abs(loss.item() - ref) < 1e-5 * max(1.0, abs(ref)), (loss.item(), ref)
    for name, p in im.unets[0].named_parameters():
        dg = float((got[name] - p.grad).abs().max())
        assert dg < 1e-4 * max(1e-3, float(p.grad.abs().max())), (name, dg, float(p.grad.abs().max()))


def test_parameter_files_round_trip(tmp_path, monkeypatch):
    from minimagen_amd.generate import load_minimagen, load_params
    from minimagen_amd.training import create_directory, get_default_args, save_training_info
    setup("emu")                                        # (load_minimagen builds engines lazily; no kernel runs here)
    monkeypatch.chdir(tmp_path)
    defaults = get_default_args(Imagen)
    assert defaults["pred_objectives"] == "noise" and defaults["min_snr_loss_weight"] is False and defaults["min_snr_gamma"] == 5.
    unet_params = [{**get_default_args(Unet), **TINY}, {**get_default_args(Unet), **TINY, "lowres_cond": True}]
    imagen_params = {**defaults, **dict(image_sizes=(16, 32), timesteps=25, text_encoder_name="t5_small", pred_objectives=("x_start", "v"),
                                        min_snr_loss_weight=(True, False), min_snr_gamma=(5., 2.5))}
    torch.manual_seed(0)
    model = Imagen([Unet(**p) for p in unet_params], **imagen_params)
    training_dir = create_directory("./training_a")
    save_training_info(types.SimpleNamespace(RESTART_DIRECTORY=None), "20260101_000000", unet_params, imagen_params, 1.0, training_dir)
    for k, u in enumerate(model.unets):
        torch.save(u.state_dict(), os.path.join("training_a", "state_dicts", f"unet_{k}_state_20260101_000000.pth"))
    _, on_disk = load_params("training_a")
    assert on_disk["pred_objectives"] == ["x_start", "v"] and on_disk["min_snr_loss_weight"] == [True, False] and on_disk["min_snr_gamma"] == [5., 2.5]
    again = load_minimagen("training_a")
    assert again.pred_objectives == ("x_start", "v") and again.min_snr_loss_weight == (True, False) and again.min_snr_gamma == (5., 2.5)
    # a directory written before the keywords existed
    old = {k: v for k, v in imagen_params.items() if k not in ("pred_objectives", "min_snr_loss_weight", "min_snr_gamma")}
    training_dir = create_directory("./training_b")
    save_training_info(types.SimpleNamespace(RESTART_DIRECTORY=None), "20260101_000001", unet_params, old, 1.0, training_dir)
    for k, u in enumerate(model.unets):
        torch.save(u.state_dict(), os.path.join("training_b", "state_dicts", f"unet_{k}_state_20260101_000001.pth"))
    assert "pred_objectives" not in json.load(open(os.path.join("training_b", "parameters", "imagen_params_20260101_000001.json")))
    older = load_minimagen("training_b")
    assert older.pred_objectives == ("noise", "noise") and older.min_snr_loss_weight == (False, False) and older.min_snr_gamma == (5., 5.)


# ------------------------------------------------------------------------------------------------ kernels
def _force(train_ops, on):
    train_ops.FORCE, train_ops.ENABLED = on, True


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("shape", [(3, 192), (2, 75), (2, 12288)])
def test_diffuse_kernel_bit_exact(backend, shape):
    """mi_diffuse_fwd through train_ops.diffuse: x_t and the target are torch.equal to the fp32 torch expressions of _p_losses / q_sample /
    calculate_v -- every objective, normalise on and off, timesteps 0 and T - 1, n % 4 != 0, more than one chunk"""
    from minimagen_amd import train_ops
    dev = setup(backend)
    B, n = shape
    T = 100
    gd = GaussianDiffusion(timesteps=T).to(dev)
    g = torch.Generator().manual_seed(n)
    x = torch.rand(B, n, generator=g).to(dev)
    eps = torch.randn(B, n, generator=g).to(dev)
    times = torch.tensor([0, T - 1, 41][:B], dtype=torch.int64).to(dev)
    assert L.lib().mi_objective_chunks(n) == (n + 4095) // 4096 and L.lib().mi_struct_size(31) == C.sizeof(L.MiDiffuseParams)
    for normalize in (True, False):
        x0 = x * 2 - 1 if normalize else x
        want_xt = gd.q_sample(x0, times, eps)
        for target in ("noise", "x_start", "v", None):
            _force(train_ops, True)
            try:
                assert train_ops.objective_active(x)
                x_t, tgt = train_ops.diffuse(x, eps, times, gd, normalize=normalize, target=target)
            finally:
                _force(train_ops, False)
            assert torch.equal(x_t, want_xt), (normalize, target)
            if target is None:
                assert tgt is None
            elif target == "noise":
                assert tgt is eps                          # no write: the caller keeps its noise
            else:
                want = x0 if target == "x_start" else gd.calculate_v(x0, times, eps)
                assert torch.equal(tgt, want), (normalize, target)
            if backend == "emu":                            # the torch-op form returns the same bits
                _force(train_ops, False)
                train_ops.ENABLED = False
                try:
                    y_t, tg2 = train_ops.diffuse(x, eps, times, gd, normalize=normalize, target=target)
                finally:
                    train_ops.ENABLED = True
                assert torch.equal(y_t, x_t) and (tgt is None or torch.equal(tg2, tgt))
    bad = torch.tensor([0, T, -1][:B], dtype=torch.int64).to(dev)            # outside [0, T): nothing is read, the image is NaN
    _force(train_ops, True)
    try:
        x_t, tgt = train_ops.diffuse(x, eps, bad, gd, normalize=True, target="v")
    finally:
        _force(train_ops, False)
    assert torch.isfinite(x_t[0]).all() and torch.isnan(x_t[1:]).all() and torch.isnan(tgt[1:]).all()
    p = L.MiDiffuseParams(B, n, T, 1, 7, x.data_ptr(), eps.data_ptr(), times.data_ptr(), 0, 0, 0)
    assert L.lib().mi_diffuse_fwd(C.byref(p), L.current_stream()) != 0


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("loss_type", LOSS_TYPES)
def test_loss_kernels_against_fp64(backend, loss_type, weighted):
    """mi_objective_loss_fwd / _bwd through train_ops.objective_loss against fp64 on the same fp32 inputs.  The only roundings: the fp32
    difference (6e-8 relative per term), the fp32 weight (exact here: the table IS fp32) and the fp32 result (6e-8); the gate is 1e-6.
    Differences on both sides of 1 (smooth-l1's two arms); n = 75 and sizes of three chunks with a ragged last one, n % 4 == 0 and not;
    two runs bit-equal; NaN reaches the loss"""
    from minimagen_amd import train_ops
    dev = setup(backend)
    T, B = 100, 3
    gd = GaussianDiffusion(timesteps=T)
    w32 = gd.loss_weight_table("v", 5.).to(dev) if weighted else None
    times = torch.tensor([0, T - 1, 37], dtype=torch.int64).to(dev)
    assert L.lib().mi_struct_size(32) == C.sizeof(L.MiObjectiveLossParams) and L.lib().mi_abi_version() == 12
    for n in (75, 8200, 9001):
        assert n == 75 or L.lib().mi_objective_chunks(n) == 3
        g = torch.Generator().manual_seed(n)
        target = torch.randn(B, n, generator=g)
        pred = target + torch.randn(B, n, generator=g) * 1.5            # |d| below and above 1
        pred[0, :4] = target[0, :4] + torch.tensor([0., 1., -1., 2.5])
        assert ((pred - target).abs() < 1).any() and ((pred - target).abs() > 1).any()
        d = (pred - target).double()                                      # the fp32 difference, as the kernel takes it
        wb = w32.cpu().double()[times.cpu()] if weighted else torch.ones(B, dtype=torch.float64)
        ref = float((wb * loss64(d, loss_type).sum(dim=1)).sum() / (B * n))
        ref_g = 0.37 * wb[:, None] * slope64(d, loss_type) / (B * n)
        runs = []
        for rep in range(2):
            p = pred.clone().to(dev).requires_grad_()                       # (a copy on the emulator too: .to() is the identity there)
            _force(train_ops, True)
            try:
                loss = train_ops.objective_loss(p, target.to(dev), times, w32, loss_type)
                (0.37 * loss).backward()
            finally:
                _force(train_ops, False)
            assert loss.shape == () and loss.dtype == torch.float32 and loss.device == p.device
            runs.append((loss.detach().cpu().clone(), p.grad.cpu().clone()))
        print(f"{loss_type} weighted={weighted} n={n}: loss {runs[0][0].item():.8f} fp64 {ref:.8f} rel {abs(runs[0][0].item() - ref) / abs(ref):.2e}")
        assert abs(runs[0][0].item() - ref) <= 1e-6 * abs(ref), (n, runs[0][0].item(), ref)
        assert ((runs[0][1].double() - ref_g).abs() <= 1e-6 * ref_g.abs() + 1e-12).all(), (n, float((runs[0][1].double() - ref_g).abs().max()))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        # the no-grad evaluation: no gradient buffer, the same loss bits
        _force(train_ops, True)
        try:
            with torch.no_grad():
                again = train_ops.objective_loss(pred.to(dev), target.to(dev), times, w32, loss_type)
            bad = pred.clone()
            bad[1, n - 1] = float("nan")
            nan_loss = train_ops.objective_loss(bad.to(dev), target.to(dev), times, w32, loss_type)
            bad[1, n - 1] = float("inf")
            inf_loss = train_ops.objective_loss(bad.to(dev), target.to(dev), times, w32, loss_type)
        finally:
            _force(train_ops, False)
        assert not again.requires_grad and torch.equal(again.cpu(), runs[0][0])
        assert torch.isnan(nan_loss).item() and torch.isinf(inf_loss).item()
        # the torch-op form of the same call (what the CPU path computes): fp32 sums, the project's loss gate
        ops = train_ops.objective_loss(pred, target, times.cpu(), None if w32 is None else w32.cpu(), loss_type)
        assert abs(ops.item() - ref) <= 1e-5 * max(1., abs(ref))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("n", [3 * 16 * 16, 75])
def test_cfg_x0_kernel_passes_an_x_start_prediction_through(backend, n):
    """mi_cfg_x0_fwd on a row (0, -1): x0 is the guided prediction to the bit, with and without guidance"""
    dev = setup(backend)
    lib = L.lib()
    B, T = 3, 100
    coef = GaussianDiffusion(timesteps=T).sampler_coef_table(objective="x_start").to(dev).contiguous()
    g = torch.Generator().manual_seed(n)
    pred2, xt = (torch.randn(2 * B, n, generator=g) * 1.5).to(dev), torch.randn(B, n, generator=g).to(dev)
    for two, scale in ((1, 3.0), (0, 1.0)):
        for t in (0, 57, T - 1):
            tstate = torch.tensor([t], dtype=torch.int32, device=dev)
            x0, pout = torch.zeros(B, n, device=dev), torch.zeros(B, n, device=dev)
            cp = L.MiCfgX0Params(B, n, pred2.data_ptr(), two, scale, xt.data_ptr(), coef.data_ptr(), tstate.data_ptr(), pout.data_ptr(), x0.data_ptr(), 0, 0)
            L.check(lib.mi_cfg_x0_fwd(C.byref(cp), L.current_stream()), "mi_cfg_x0_fwd")
            c, nl = pred2[:B], pred2[B:]
            want = nl + (c - nl) * scale if two else c
            assert torch.equal(pout, want) and torch.equal(x0, want), (two, t)


def _loss_grads(im, imgs, emb, mask, hip, unet_number, grad=True):
    from minimagen_amd import train_ops
    train_ops.FORCE, train_ops.ENABLED = hip, hip
    try:
        im.zero_grad(set_to_none=True)
        torch.manual_seed(11)                                           # the same timesteps / noise / dropout mask on both paths
        if not grad:
            with torch.no_grad():
                return im(imgs, text_embeds=emb, text_masks=mask, unet_number=unet_number).item(), None
        loss = im(imgs, text_embeds=emb, text_masks=mask, unet_number=unet_number)
        loss.backward()
        return loss.item(), {n: p.grad.clone() for n, p in im.unets[unet_number - 1].named_parameters()}
    finally:
        train_ops.FORCE, train_ops.ENABLED = False, True


@pytest.mark.parametrize("backend", BACKENDS)
def test_training_step_on_the_device_path_equals_the_torch_op_path(backend):
    """tests/test_training.py's test of the same name for pred_objectives = ('x_start', 'v') with the min-SNR weight: the front and the loss on
    objective.hip (and the U-Net on its HIP training graph) against the torch-op path, the same two gates; and the no-grad evaluation of the
    loss (train mode, same seed) against the train-mode loss to 2e-5 relative"""
    from minimagen_amd import train_ops
    dev = setup(backend)
    torch.manual_seed(7)
    size = (16, 32) if backend == "emu" else (32, 64)
    im = Imagen((Unet(**BASE), Unet(**SR)), text_encoder_name="t5_small", image_sizes=size, timesteps=60, pred_objectives=("x_start", "v"),
                min_snr_loss_weight=True).train().to(dev)
    imgs = torch.rand(2, 3, size[1] + 8, size[1] + 8, device=dev)
    emb, mask = R.synthetic_text(2, length=11, seed=5)
    emb, mask = emb.to(dev), mask.to(dev)
    calls = []
    real = train_ops._ObjectiveLossFn.apply
    for n in (1, 2):
        la, ga = _loss_grads(im, imgs, emb, mask, False, n)
        train_ops._ObjectiveLossFn.apply = staticmethod(lambda *a: (calls.append(n), real(*a))[1])
        try:
            lb, gb = _loss_grads(im, imgs, emb, mask, True, n)
            lc, _ = _loss_grads(im, imgs, emb, mask, True, n, grad=False)
        finally:
            train_ops._ObjectiveLossFn.apply = real
        print(f"unet {n}: torch ops {la:.7f}, device {lb:.7f}, device no-grad {lc:.7f}")
        assert abs(la - lb) < 1e-5 * max(1.0, abs(la)), (la, lb)
        for name, g in ga.items():
            assert (gb[name] - g).abs().max() < 1e-4 * max(1e-3, float(g.abs().max())), (n, name, float((gb[name] - g).abs().max()), float(g.abs().max()))
        assert abs(lc - lb) <= 2e-5 * abs(lb), (lb, lc)
    assert calls == [1, 1, 2, 2]                      # the device route was taken, with and without autograd


# ------------------------------------------------------------------------------------------------ sampling against a restated loop
def make_imagen(sizes, T, dev, objectives, cond_drop_prob=0.15):
    p = I.unet_params()
    unets = [Unet(**p["unet0"])] + [Unet(**p["unet1"]) for _ in sizes[1:]]
    extra = {} if objectives is None else dict(pred_objectives=objectives)
    im = Imagen(unets, text_encoder_name="t5_small", image_sizes=sizes, timesteps=T, cond_drop_prob=cond_drop_prob, **extra)
    im.unets[0].load_state_dict(I.load("unet0_sd.pt"))
    for u in im.unets[1:]:
        u.load_state_dict(I.load("unet1_sd.pt"))
    return im.to(dev)


def restated_sample(sds, sizes, T, steps, sampler, objectives, *, text_embeds, text_masks, cond_scale, randn, inpaint=None, lowres_sample_noise_level=0.2):
    """the loop of tests/test_sample_steps.py::restated_sample (``steps`` None: the default loop on sampler_coef_table) on a table whose columns
    0 and 1 are rebuilt HERE in fp64 from the betas for the stage's objective -- the U-Net's output is read as that prediction; ``inpaint`` =
    (images, masks) at the stage's size: the known region as tests/test_inpaint.py restates it"""
    from oracle import resize_restated
    b = text_embeds.shape[0]
    steps = (steps,) * len(sds) if (steps is None or isinstance(steps, int)) else steps
    lowres_sched = R.Schedule(T)
    gd = GaussianDiffusion(timesteps=T)
    img = None
    for sd, size, S, objective in zip(sds, sizes, steps, objectives):
        kw = dict(text_embeds=text_embeds, text_mask=text_masks, cond_scale=cond_scale)
        if "to_lowres_time_hiddens.1.weight" in sd:
            lt = lowres_sched.get_times(b, lowres_sample_noise_level)
            low = resize_restated.resize(img, scale_factors=size / img.shape[-1], pad_mode='reflect') if img.shape[-1] != size else img
            low = lowres_sched.q_sample(low, int(lt[0]), randn(low.shape))
            kw.update(lowres_cond_img=low * 2 - 1, lowres_noise_times=lt)
        known = {} if inpaint is None else dict(known=True)
        if S is None:
            S, tau, tab = T, torch.arange(T), gd.sampler_coef_table(**known)
        else:
            tau, tab = gd.sampler_tables(S, sampler, None, **known)
        tab = tab.clone()
        tab[:, :2] = columns64(abar64(T)[tau], objective).to(torch.float32)
        shape = (b, 3, size, size)
        x, prev = randn(shape), torch.zeros(shape)
        zs = [randn(shape) for _ in range(S)]
        if inpaint is not None:
            y, m = inpaint[0].clamp(0., 1.) * 2 - 1, inpaint[1][:, None] != 0
            ks = [randn(shape) for _ in range(S)]
            a0, b0 = abar64(T)[-1].sqrt().to(torch.float32), (1. - abar64(T)[-1]).sqrt().to(torch.float32)
            x = torch.where(m, a0 * y + b0 * ks[0], x)
        for k in range(S - 1, -1, -1):
            pred = R.unet_forward_with_cond_scale(sd, x, torch.full((b,), int(tau[k]), dtype=torch.long), **kw)
            x0 = tab[k, 0] * x - tab[k, 1] * pred
            s, *_ = R.dynamic_threshold_quantile(x0.reshape(b, -1).abs(), 0.9)
            s = s.clamp(min=1.).reshape(b, 1, 1, 1)
            x0 = x0.clamp(-s, s) / s
            x = ((tab[k, 2] * x0 + tab[k, 3] * x) + tab[k, 5] * prev) + tab[k, 4] * zs[S - 1 - k]
            prev = x0
            if inpaint is not None:
                x = torch.where(m, tab[k, 6] * y + tab[k, 7] * ks[S - k] if k > 0 else y, x)
        img = (x.clamp(-1., 1.) + 1) * 0.5
    return img


def gate(out, ref, what):
    d = (out.cpu() - ref).abs()
    print(f"{what}: max|d| = {d.max():.2e}, mean|d| = {d.mean():.2e}")
    assert out.shape == ref.shape and torch.isfinite(out).all()
    assert d.max() < 1e-4 and d.mean() < 1e-5, (what, d.max(), d.mean())


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("sampler", ["ddpm", "dpmpp_2m"])
@pytest.mark.parametrize("objective", ["v", "x_start"])
def test_values_small(backend, objective, sampler):
    """32^2, B = 2, T = 100, S = 6, cond_scale 3, golden base weights read as a v / x_start predictor"""
    dev = setup(backend)
    im = make_imagen([32], 100, dev, objective)
    emb, mask = R.synthetic_text(2, length=16, seed=7)
    out = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., _noise=R.make_randn(3), sample_steps=6, sampler=sampler)
    ref = restated_sample([I.load("unet0_sd.pt")], [32], 100, 6, sampler, [objective], text_embeds=emb, text_masks=mask, cond_scale=3., randn=R.make_randn(3))
    gate(out, ref, f"{backend} 32^2 T=100 S=6 {sampler} {objective}")
    im.check_device_status()
    keys = [k for u in im.unets for ws in u.engine()._ws.values() for k in ws.sampler_state]
    assert keys == [(100, 6, sampler, 1. if sampler == "ddpm" else 0., objective)]


@pytest.mark.parametrize("backend", GPU_ONLY)
def test_values_base_stage_v(backend):
    """base 64^2, cond_scale 3, T = 100, S = 20, B = 2, 'v'"""
    dev = setup(backend)
    im = make_imagen([64], 100, dev, "v")
    emb, mask = R.synthetic_text(2, length=48, seed=9)
    for sampler in ("ddpm", "dpmpp_2m"):
        out = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., _noise=R.make_randn(21), sample_steps=20, sampler=sampler)
        ref = restated_sample([I.load("unet0_sd.pt")], [64], 100, 20, sampler, ["v"], text_embeds=emb, text_masks=mask, cond_scale=3., randn=R.make_randn(21))
        gate(out, ref, f"base 64^2 T=100 S=20 {sampler} v")
        im.check_device_status()


@pytest.mark.parametrize("backend", GPU_ONLY)
def test_values_default_loop_v(backend):
    """the full default loop (no sample_steps: the reference's table with columns 0 and 1 of 'v'), 32^2, T = 100"""
    dev = setup(backend)
    im = make_imagen([32], 100, dev, "v")
    emb, mask = R.synthetic_text(2, length=16, seed=7)
    out = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., _noise=R.make_randn(5))
    ref = restated_sample([I.load("unet0_sd.pt")], [32], 100, None, None, ["v"], text_embeds=emb, text_masks=mask, cond_scale=3., randn=R.make_randn(5))
    gate(out, ref, "32^2 T=100 default loop v")
    im.check_device_status()
    keys = [k for u in im.unets for ws in u.engine()._ws.values() for k in ws.sampler_state]
    assert keys == [(100, "v")]


@pytest.mark.parametrize("backend", GPU_ONLY)
def test_values_cascade_v(backend):
    """64 -> 256, T = 100, sample_steps = (25, 10), objectives ('v', 'v'): the grouped tail on the 256^2 stage"""
    dev = setup(backend)
    im = make_imagen([64, 256], 100, dev, ("v", "v"))
    emb, mask = R.synthetic_text(2, length=48, seed=9)
    out = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., _noise=R.make_randn(21), sample_steps=(25, 10), sampler="dpmpp_2m")
    ref = restated_sample([I.load("unet0_sd.pt"), I.load("unet1_sd.pt")], [64, 256], 100, (25, 10), "dpmpp_2m", ["v", "v"], text_embeds=emb, text_masks=mask,
                          cond_scale=3., randn=R.make_randn(21))
    gate(out, ref, "cascade 64->256 T=100 S=(25, 10) dpmpp_2m v")
    im.check_device_status()
    st = [v for u in im.unets for ws in u.engine()._ws.values() for v in ws.sampler_state.values()]
    assert [hasattr(v, "group_sync") for v in st].count(True) == 1


@pytest.mark.parametrize("backend", GPU_ONLY)
def test_values_inpaint_v(backend):
    """one inpainting call at 32^2 (images given at the stage's size), T = 100, S = 6, 'v'"""
    dev = setup(backend)
    im = make_imagen([32], 100, dev, "v")
    emb, mask = R.synthetic_text(2, length=16, seed=7)
    g = torch.Generator().manual_seed(5)
    y, m = torch.rand(2, 3, 32, 32, generator=g), torch.rand(2, 32, 32, generator=g) < 0.5
    out = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., _noise=R.make_randn(3), sample_steps=6, sampler="ddpm",
                    inpaint_images=y.to(dev), inpaint_masks=m.to(dev))
    ref = restated_sample([I.load("unet0_sd.pt")], [32], 100, 6, "ddpm", ["v"], text_embeds=emb, text_masks=mask, cond_scale=3., randn=R.make_randn(3), inpaint=(y, m))
    gate(out, ref, "32^2 T=100 S=6 ddpm v inpaint")
    im.check_device_status()


@pytest.mark.parametrize("backend", BACKENDS)
def test_noise_objective_is_untouched(backend):
    """a model built with pred_objectives='noise' samples torch.equal to one built without the keyword, and the stage-state store of a
    default model holds the keys it held before the keyword existed.  The emulator (~1 s per step) compares a two-step solver call only; the
    default loop's key on it is pinned by tests/test_sample_steps.py::test_default_call_is_untouched"""
    dev = setup(backend)
    gpu = backend == "gpu"
    T, S = (25, 5) if gpu else (21, 2)                  # (T = 20 has abar = 0 at the last timestep: the noise objective divides by it)
    emb, mask = R.synthetic_text(2, length=10, seed=3)
    outs = []
    for objectives in (None, "noise"):
        torch.manual_seed(4)
        extra = {} if objectives is None else dict(pred_objectives=objectives)
        im = Imagen([Unet(**dict(TINY, memory_efficient=True))], text_encoder_name="t5_small", image_sizes=[16], timesteps=T, cond_drop_prob=0.15, **extra).to(dev)
        kw = dict(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., _seed=11)
        b = im.sample(**kw, sample_steps=S, sampler="dpmpp_2m").clone()
        a = im.sample(**kw).clone() if gpu else None
        outs.append((a, b))
        keys = [k for u in im.unets for ws in u.engine()._ws.values() for k in ws.sampler_state]
        assert keys == [(T, S, "dpmpp_2m", 0.)] + ([T] if gpu else [])
        im.check_device_status()
    assert torch.equal(outs[0][1], outs[1][1]) and (not gpu or torch.equal(outs[0][0], outs[1][0]))
    assert outs[1][1].isfinite().all() and outs[1][1].std() > 0.01
