"""The wide presets' attention core in the training graph (attn_train_wide.hip: mi_flash_attn_train_fwd / _bwd, train_ops.flash_attention):
kernels against fp64 autograd, the forward against the inference kernel, determinism, the layers and a U-Net against their torch-op forms,
memory, the fallback for what the kernels do not cover, and no scratch in the new kernels."""
import ctypes as C
import os

import pytest
import torch

from minimagen_amd import _lib as L
from minimagen_amd import packing as P
from minimagen_amd import train_ops
from oracle import restated as R
from tests._backend import BACKENDS, GPU_ONLY, setup


def _inputs(B, n, H, J, kvh, masked, e=0, seed=3):
    """q, k, v, mask, dout and the softmax scale; operands 2^e / 2^-e / 2^(e/2) off unit with the logits kept O(1)"""
    g = torch.Generator().manual_seed(seed)
    qs, ks, vs = 2.0 ** e, 2.0 ** (-e if e > 0 else e // 2), 2.0 ** (e // 2)
    q = torch.randn(B, n, H * 64, generator=g) * qs
    k = torch.randn(B, J, kvh * 64, generator=g) * ks
    v = torch.randn(B, J, kvh * 64, generator=g) * vs
    mask = None
    if masked:
        mask = torch.arange(J)[None, :] < torch.tensor([J - (5 * r + 3) % (J - 1) for r in range(B)])[:, None]
        mask[:, 0] = True                            # the null row
    dout = torch.randn(B, n, H * 64, generator=g) * 2.0 ** (e // 3)
    return q, k, v, mask, dout, 64 ** -0.5 / (qs * ks)


def _reference(q, k, v, mask, dout, scale):
    """fp64 autograd of softmax(scale q k^T) v per head: out, dq, dk, dv"""
    B, n, inner = q.shape
    H, J, kvh = inner // 64, k.shape[1], k.shape[2] // 64
    qd, kd, vd = (t.double().requires_grad_() for t in (q, k, v))
    qh = qd.reshape(B, n, H, 64).transpose(1, 2)
    kh = kd.reshape(B, J, kvh, 64).transpose(1, 2).expand(B, H, J, 64)
    vh = vd.reshape(B, J, kvh, 64).transpose(1, 2).expand(B, H, J, 64)
    sim = qh @ kh.transpose(-1, -2) * scale
    if mask is not None:
        sim = sim.masked_fill(~mask[:, None, None, :], -torch.finfo(torch.float32).max)
    out = (sim.softmax(-1) @ vh).transpose(1, 2).reshape(B, n, inner)
    out.backward(dout.double())
    return [out.detach(), qd.grad, kd.grad, vd.grad]


def _device(q, k, v, mask, dout, scale, dev):
    train_ops.FORCE = True
    try:
        qq, kk, vv = (t.to(dev).requires_grad_() for t in (q, k, v))
        out = train_ops.flash_attention(qq, kk, vv, None if mask is None else mask.to(dev), scale)
        out.backward(dout.to(dev))
    finally:
        train_ops.FORCE = False
    return [t.detach().cpu() for t in (out, qq.grad, kk.grad, vv.grad)]


CASES = [(2, 70, 8, 71, 1, False, 0), (1, 300, 4, 301, 1, False, 0), (3, 129, 8, 37, 8, True, 0), (2, 70, 8, 71, 1, True, 0),
         (2, 45, 8, 71, 1, False, -8), (2, 45, 8, 71, 1, False, 6), (2, 33, 4, 20, 4, True, -6), (1, 50, 2, 130, 2, True, 5)]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", CASES)
def test_flash_train_kernels_against_fp64_autograd(backend, case):
    """out, dq, dk, dv of mi_flash_attn_train_fwd / _bwd against torch autograd in fp64: multi-query and per-head k / v, ragged key masks, token
    counts that are no multiple of 16 or 64, head counts that are no multiple of four, operands 2^-8 .. 2^6 off unit"""
    dev = setup(backend)
    *x, scale = _inputs(*case)
    want = _reference(*x, scale)
    got = _device(*x, scale, dev)
    for name, a, r in zip(("out", "dq", "dk", "dv"), got, want):
        err = float((a.double() - r).abs().max())
        assert err < 3e-5 * max(1.0, float(r.abs().max())), (case, name, err, float(r.abs().max()))


@pytest.mark.parametrize("case", [(2, 4096, 8, 4097), (4, 1024, 8, 1025)])
@pytest.mark.parametrize("backend", GPU_ONLY)
def test_flash_train_kernels_at_the_wide_presets_shapes(backend, case):
    """the self-attention shapes of Unet() default at 64 x 64 (4096 tokens) and of Base / Super (1024 tokens), multi-query, against fp64 on the GPU"""
    dev = setup(backend)
    B, n, H, J = case
    q, k, v, mask, dout, scale = _inputs(B, n, H, J, 1, False)
    want = _reference(*(t.to(dev) for t in (q, k, v)), None, dout.to(dev), scale)
    got = _device(q, k, v, None, dout, scale, dev)
    for name, a, r in zip(("out", "dq", "dk", "dv"), got, want):
        r = r.cpu()
        err = float((a.double() - r).abs().max())
        assert err < 3e-5 * max(1.0, float(r.abs().max())), (case, name, err, float(r.abs().max()))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", [(2, 70, 8, 71, 1), (1, 300, 4, 301, 1), (3, 129, 8, 37, 8)])
def test_flash_train_forward_is_the_inference_kernel(backend, case):
    """unmasked, the training forward's output is mi_flash_attn_fwd's (prepared K / V, one context segment, no separate null row) to the bit"""
    dev = setup(backend)
    B, n, H, J, kvh = case
    q, k, v, _, _, scale = _inputs(B, n, H, J, kvh, False)
    q, k, v = q.to(dev), k.to(dev), v.to(dev)
    train_ops.FORCE = True
    try:
        with torch.no_grad():
            out = train_ops.flash_attention(q, k, v, None, scale)
    finally:
        train_ops.FORCE = False
    lib = L.lib()
    ref = torch.empty_like(q)
    prep = torch.empty(lib.mi_flash_kv_prep_bytes(B * kvh, J), dtype=torch.uint8, device=dev)
    p = L.MiFlashAttnParams()
    p.B, p.HW, p.heads, p.kv_heads, p.q, p.q_scale = B, n, H, kvh, q.data_ptr(), scale * P.LOG2E
    p.k0, p.v0, p.n0, p.ld0, p.bs0 = k.data_ptr(), v.data_ptr(), J, kvh * 64, J * kvh * 64
    p.out, p.kv_prep, p.kv_prep_bytes = ref.data_ptr(), prep.data_ptr(), prep.numel()
    L.check(lib.mi_flash_attn_fwd(C.byref(p), L.current_stream()), "mi_flash_attn_fwd")
    assert torch.equal(out, ref)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", [(1, 300, 4, 301, 1, False, 0), (3, 129, 8, 37, 8, True, 0)])
def test_flash_train_backward_is_deterministic(backend, case):
    """two backward runs give the same dq, dk and dv to the bit (the query splits' dk / dv partials are added in a fixed order)"""
    dev = setup(backend)
    *x, scale = _inputs(*case)
    a = _device(*x, scale, dev)
    b = _device(*x, scale, dev)
    for u, w in zip(a[1:], b[1:]):
        assert torch.equal(u, w)


def _layer_grads(layer, args, gy, flash):
    prev = train_ops.FORCE, train_ops.FLASH_TRAIN
    train_ops.FORCE, train_ops.FLASH_TRAIN = True, flash         # (the rest of the layer on the device path both times)
    try:
        inputs = [a for a in (args[0], args[1].get("context")) if a is not None]
        for t in list(layer.parameters()) + inputs:
            t.grad = None
        y = layer(*args[:1], **args[1])
        y.backward(gy)
        return [y.detach().cpu().clone()] + [a.grad.detach().cpu().clone() for a in inputs] + \
            [p_.grad.detach().cpu().clone() for p_ in layer.parameters() if p_.grad is not None], [n_ for n_, p_ in layer.named_parameters() if p_.grad is not None]
    finally:
        train_ops.FORCE, train_ops.FLASH_TRAIN = prev


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("kind", ["attn64", "attn128_ctx", "attn128_masked_ctx", "cross64", "cross128"])
def test_flash_train_layers_equal_the_torch_op_form(backend, kind):
    """Attention (multi-query, with and without a context) and CrossAttention (a k / v head per head, masked context) with the core on the flash
    kernels against the layers' torch-op forms: output, input and context gradients and every parameter gradient (null_kv, to_q, to_kv,
    to_context, to_out, the norms)"""
    from minimagen_amd.layers import Attention, CrossAttention
    dev = setup(backend)
    torch.manual_seed(5)
    dim = 64 if kind.endswith("64") else 128
    B, n, Jc, cd = 2, 77, 9, 96
    if kind.startswith("attn"):
        layer = Attention(dim=dim, context_dim=cd if "ctx" in kind else None)
    else:
        layer = CrossAttention(dim=dim, context_dim=cd, norm_context=True)
    with torch.no_grad():
        for p_ in layer.parameters():
            p_.add_(0.1 * torch.randn_like(p_))
    layer = layer.train().to(dev)
    x = torch.randn(B, n, dim).to(dev).requires_grad_()
    kw = {}
    if "ctx" in kind or kind.startswith("cross"):
        kw["context"] = torch.randn(B, Jc, cd).to(dev).requires_grad_()
    if "masked" in kind or kind.startswith("cross"):
        m = torch.arange(Jc)[None, :] < torch.tensor([Jc, 4])[:, None]
        kw["mask"] = (torch.cat((m, torch.ones(B, n, dtype=torch.bool)), dim=1) if kind.startswith("attn") else m).to(dev)   # (context rows first)
    gy = torch.randn(B, n, dim).to(dev)
    calls = []
    real = train_ops._FlashAttnFn.apply
    train_ops._FlashAttnFn.apply = lambda *a: calls.append(a[1].shape[-1]) or real(*a)
    try:
        got, names = _layer_grads(layer, [x, kw], gy, True)
    finally:
        train_ops._FlashAttnFn.apply = real
    assert calls == [64 if kind.startswith("attn") else 8 * 64]
    want, names_ref = _layer_grads(layer, [x, kw], gy, False)
    assert names == names_ref and len(got) == len(want)
    labels = ["out", "x"] + (["context"] if "context" in kw else []) + names
    for label, a, b in zip(labels, got, want):
        err = float((a - b).abs().max())
        assert err <= 2e-5 * max(1e-3, float(b.abs().max())), (kind, label, err, float(b.abs().max()))


def _unet_loss_grads(im, imgs, emb, mask, flash):
    prev = train_ops.FORCE, train_ops.FLASH_TRAIN
    train_ops.FORCE = imgs.device.type == "cpu" or prev[0]
    train_ops.FLASH_TRAIN = flash
    try:
        im.zero_grad(set_to_none=True)
        torch.manual_seed(11)
        loss = im(imgs, text_embeds=emb, text_masks=mask, unet_number=1)
        loss.backward()
        return loss.item(), {n: p.grad.clone() for n, p in im.unets[0].named_parameters()}
    finally:
        train_ops.FORCE, train_ops.FLASH_TRAIN = prev


def _unet_check(dev, unet_kw, size, B):
    from minimagen_amd.Imagen import Imagen
    from minimagen_amd.Unet import Unet
    torch.manual_seed(8)
    im = Imagen((Unet(**unet_kw),), text_encoder_name="t5_small", image_sizes=(size,), timesteps=60).train().to(dev)
    imgs = torch.rand(B, 3, size, size, device=dev)
    emb, mask = R.synthetic_text(B, length=11, seed=5)
    emb, mask = emb.to(dev), mask.to(dev)
    calls = []
    real = train_ops._FlashAttnFn.apply
    train_ops._FlashAttnFn.apply = lambda *a: calls.append((a[0].shape[-1], a[1].shape[-1])) or real(*a)
    try:
        lb, gb = _unet_loss_grads(im, imgs, emb, mask, True)
    finally:
        train_ops._FlashAttnFn.apply = real
    assert any(kv == 64 for _, kv in calls) and any(kv == qd > 64 for qd, kv in calls), calls      # the multi-query Attention and the CrossAttention
    la, ga = _unet_loss_grads(im, imgs, emb, mask, False)
    assert abs(la - lb) < 1e-5 * max(1.0, abs(la)), (la, lb)
    for name, g in ga.items():
        assert (gb[name] - g).abs().max() < 1e-4 * max(1e-3, float(g.abs().max())), (name, float((gb[name] - g).abs().max()), float(g.abs().max()))


@pytest.mark.parametrize("backend", BACKENDS)
def test_flash_train_unet_step_equals_the_torch_op_path(backend):
    """Imagen.forward -> loss.backward() of a U-Net with wide self- and cross-attention at every level and in the middle: the flash core (the
    rest of the device path as it is) against MINIMAGEN_FLASH_TRAIN=0's torch-op attention: the loss and every gradient"""
    dev = setup(backend)
    kw = dict(dim=64, dim_mults=(1, 2), num_resnet_blocks=1, layer_attns=True, layer_cross_attns=True, attend_at_middle=True)
    _unet_check(dev, kw, 16 if backend == "emu" else 32, 2)


@pytest.mark.parametrize("backend", GPU_ONLY)
def test_flash_train_default_unet_step_equals_the_torch_op_path(backend):
    """the same for Unet() default at 64 x 64 (self-attention over 4096 tokens), B = 2"""
    _unet_check(setup(backend), {}, 64, 2)


@pytest.mark.gpu
def test_flash_train_layer_memory():
    """one Attention(dim=128) over 4096 tokens at B = 4, forward + backward: the peak grows by less than 0.5 GB (the torch-op form keeps two
    [4, 8, 4096, 4097] fp32 tensors: > 4.3 GB)"""
    from minimagen_amd.layers import Attention
    dev = setup("gpu")
    torch.manual_seed(2)
    layer = Attention(dim=128).train().to(dev)
    x = torch.randn(4, 4096, 128, device=dev, requires_grad=True)
    gy = torch.randn(4, 4096, 128, device=dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    layer(x).backward(gy)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - base
    assert grew < 0.5 * 2 ** 30, grew / 2 ** 30


def test_flash_train_support_test_keeps_other_attention_on_torch_ops():
    """an Attention with dim_head 32 (the kernels are dim_head 64), or with an attn_bias, never reaches the flash kernels: the same results as
    the torch-op form, to the bit"""
    from minimagen_amd.layers import Attention
    setup("emu")
    torch.manual_seed(6)
    x = torch.randn(2, 40, 64)
    for layer, bias in ((Attention(dim=64, dim_head=32), None), (Attention(dim=64), torch.randn(2, 8, 40, 41))):
        res = []
        for flash in (True, False):
            train_ops.FORCE, train_ops.FLASH_TRAIN = True, flash
            try:
                xx = x.clone().requires_grad_()
                layer.zero_grad(set_to_none=True)
                y = layer(xx, attn_bias=bias)
                y.sum().backward()
                res.append([y.detach(), xx.grad] + [p_.grad for p_ in layer.parameters()])
            finally:
                train_ops.FORCE, train_ops.FLASH_TRAIN = False, True
        assert not train_ops.flash_attention_supported(x, layer.null_kv.shape[-1], bias)
        for a, b in zip(*res):
            assert torch.equal(a, b)


def test_flash_train_kernels_use_no_scratch():
    """no kernel of attn_train_wide.hip (and no training instantiation of the shared forward) spills to scratch"""
    import shutil
    import subprocess
    import tempfile
    from tools.check_code_objects import OBJDUMP, READELF, kernel_scratch
    if not (os.path.exists(OBJDUMP) and os.path.exists(READELF)):
        pytest.skip("llvm-objdump not available")
    d = tempfile.mkdtemp(prefix="mi_flash_scratch_")
    try:
        shutil.copy(L.DEFAULT_LIB, os.path.join(d, "lib.so"))
        subprocess.run([OBJDUMP, "--offloading", "lib.so"], cwd=d, check=True, capture_output=True)
        found = {}
        for f in sorted(x for x in os.listdir(d) if "gfx950" in x):
            for name, scratch in kernel_scratch(os.path.join(d, f)).items():
                if "flash_bwd_" in name or ("flash_attn_mq_kernel" in name and "ELb1EEEv" in name):
                    found[name] = scratch
    finally:
        shutil.rmtree(d, ignore_errors=True)
    assert len([n for n in found if "flash_bwd_" in n]) >= 5, found
    assert all(v == 0 for v in found.values()), found
