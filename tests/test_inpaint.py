"""Imagen.sample(inpaint_images=, inpaint_masks=, start_image=, start_at_stage=, stop_at_stage=): conditioning the sampler on pixels the
caller has.  The tables (columns 6 and 7), the kernels (the masked replace in the three sampler tails, blend 0, the Philox streams), the
invariants of the sampling loop (empty mask == plain call, full mask == known image, sharding, graph reuse) and the values against a
restated loop on injected noise (the project's gate, SURVEY.md 8(c): max|d| < 1e-4 and mean|d| < 1e-5 on [0, 1] images)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from minimagen_amd import _lib as L
from minimagen_amd.Imagen import Imagen
from minimagen_amd.Unet import Unet
from minimagen_amd.diffusion_model import GaussianDiffusion
from minimagen_amd.helpers import quantile_rank
from oracle import resize_restated
from oracle import restated as R
from tests import _inputs as I
from tests._backend import BACKENDS, GPU_ONLY, setup
from tests.test_sample_steps import SOLVERS, TINY, gate, make_imagen, tiny_imagen

KNOWN_STREAM = 3 << 18
MI_ERR_INVALID = -1


def pixels(B, size, seed, lo=0., hi=1.):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, 3, size, size, generator=g) * (hi - lo) + lo


def masks_half_and_random(B, size, seed):
    """row 0: the left half-plane is known; the other rows: a random half of the pixels"""
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(B, size, size, generator=g) < 0.5
    m[0] = torch.arange(size)[None, :] < size // 2
    return m


def restated_inpaint_sample(sds, sizes, T, steps, sampler, eta, *, images, masks, text_embeds, text_masks, cond_scale, randn,
                            lowres_sample_noise_level=0.2):
    """tests.test_sample_steps.restated_sample with the known region: per stage the draw order is low-resolution noise, x_T, the S step
    draws, the S known-region draws; blend 0 behind x_T, blend s + 1 behind the step counted s from the first (row 0: no draw, y itself);
    ``steps`` None: the default loop on sampler_coef_table"""
    b = text_embeds.shape[0]
    steps = (steps,) * len(sds) if (steps is None or isinstance(steps, int)) else steps
    lowres_sched = R.Schedule(T)
    gd = GaussianDiffusion(timesteps=T)
    img = None
    for sd, size, S in zip(sds, sizes, steps):
        kw = dict(text_embeds=text_embeds, text_mask=text_masks, cond_scale=cond_scale)
        if "to_lowres_time_hiddens.1.weight" in sd:
            lt = lowres_sched.get_times(b, lowres_sample_noise_level)
            low = resize_restated.resize(img, scale_factors=size / img.shape[-1], pad_mode='reflect') if img.shape[-1] != size else img
            low = lowres_sched.q_sample(low, int(lt[0]), randn(low.shape))
            kw.update(lowres_cond_img=low * 2 - 1, lowres_noise_times=lt)
        if S is None:
            S, tau, tab = T, torch.arange(T), gd.sampler_coef_table(known=True)
        else:
            tau, tab = gd.sampler_tables(S, sampler, eta, known=True)
        y = resize_restated.resize(images, scale_factors=size / images.shape[-1], pad_mode='reflect') if images.shape[-1] != size else images
        y = y.clamp(0., 1.) * 2 - 1
        m = F.interpolate(masks.float()[:, None], size=(size, size), mode='nearest') != 0
        shape = (b, 3, size, size)
        x, prev = randn(shape), torch.zeros(shape)
        zs = [randn(shape) for _ in range(S)]
        ks = [randn(shape) for _ in range(S)]
        a0, b0 = gd.known_start_coefs()
        x = torch.where(m, a0 * y + b0 * ks[0], x)
        for k in range(S - 1, -1, -1):
            pred = R.unet_forward_with_cond_scale(sd, x, torch.full((b,), int(tau[k]), dtype=torch.long), **kw)
            x0 = tab[k, 0] * x - tab[k, 1] * pred
            s, *_ = R.dynamic_threshold_quantile(x0.reshape(b, -1).abs(), 0.9)
            s = s.clamp(min=1.).reshape(b, 1, 1, 1)
            x0 = x0.clamp(-s, s) / s
            x = ((tab[k, 2] * x0 + tab[k, 3] * x) + tab[k, 5] * prev) + tab[k, 4] * zs[S - 1 - k]
            prev = x0
            x = torch.where(m, tab[k, 6] * y + tab[k, 7] * ks[S - k] if k > 0 else y, x)
        img = (x.clamp(-1., 1.) + 1) * 0.5
    return img


# ------------------------------------------------------------------------------------------------ 1. tables (host)
@pytest.mark.parametrize("T,S", [(100, 10), (100, 100), (1000, 50), (25, 2)])
@pytest.mark.parametrize("sampler,eta", SOLVERS)
def test_known_columns(T, S, sampler, eta):
    gd = GaussianDiffusion(timesteps=T)
    tau, a, tab = gd._sampler_tables64(S, sampler, eta, known=True)
    betas = torch.linspace(1000 / T * 0.0001, 1000 / T * 0.02, T, dtype=torch.float64)
    abar = torch.cumprod(1. - betas, dim=0)
    ap = torch.cat([torch.ones(1, dtype=torch.float64), abar[tau[:-1]]])          # abar at tau_{k-1}, abar_{-1} = 1
    assert tab.dtype == torch.float64 and (tab[:, 6] ** 2 + tab[:, 7] ** 2 - 1).abs().max() < 1e-14
    assert torch.equal(tab[:, 6], ap.sqrt())
    plain64 = gd._sampler_tables64(S, sampler, eta)[2]
    assert torch.equal(plain64[:, :6], tab[:, :6]) and (plain64[:, 6:] == 0).all()
    tau32, tab32 = gd.sampler_tables(S, sampler, eta, known=True)
    plain = gd.sampler_tables(S, sampler, eta)[1]
    assert tab32.dtype == torch.float32 and torch.equal(tab32, tab.to(torch.float32)) and torch.equal(tau32, tau)
    assert tab32[0, 6] == 1 and tab32[0, 7] == 0
    assert torch.equal(tab32[:, :6].view(torch.int32), plain[:, :6].view(torch.int32)) and (plain[:, 6:] == 0).all()
    # the default loop's table builder
    d, dk = gd.sampler_coef_table(), gd.sampler_coef_table(known=True)
    assert torch.equal(d[:, :6].view(torch.int32), dk[:, :6].view(torch.int32)) and (d[:, 6:] == 0).all()
    apT = torch.cat([torch.ones(1, dtype=torch.float64), abar[:-1]])
    assert torch.equal(dk[:, 6], apT.sqrt().to(torch.float32)) and torch.equal(dk[:, 7], (1 - apT).sqrt().to(torch.float32))
    assert dk[0, 6] == 1 and dk[0, 7] == 0
    a0, b0 = gd.known_start_coefs()
    assert a0 == float(abar[-1].sqrt().to(torch.float32)) and b0 == float((1 - abar[-1]).sqrt().to(torch.float32))


# ------------------------------------------------------------------------------------------------ 2. argument validation (host)
def test_argument_validation():
    """bad or inconsistent values raise ValueError before anything is launched (no backend is loaded here: a launch would need one)"""
    im = Imagen([Unet(**TINY), Unet(**TINY, lowres_cond=True)], text_encoder_name="t5_small", image_sizes=[16, 32], timesteps=25, cond_drop_prob=0.15)
    emb, mask = R.synthetic_text(2, length=8, seed=1)
    img, m = torch.rand(2, 3, 32, 32), torch.ones(2, 32, 32, dtype=torch.bool)
    bad = [dict(inpaint_masks=m),                                                    # masks without images
           dict(inpaint_images=img),                                                 # images without masks
           dict(inpaint_images=torch.rand(3, 3, 32, 32), inpaint_masks=torch.ones(3, 32, 32, dtype=torch.bool)),      # batch != text batch
           dict(inpaint_images=img, inpaint_masks=torch.ones(3, 32, 32, dtype=torch.bool)),
           dict(inpaint_images=torch.rand(2, 4, 32, 32), inpaint_masks=m),          # channel count
           dict(inpaint_images=torch.rand(2, 3, 32, 24), inpaint_masks=m),          # not square
           dict(inpaint_images=img, inpaint_masks=torch.full((2, 32, 32), 2)),      # mask values other than 0 / 1
           dict(inpaint_images=img, inpaint_masks=torch.full((2, 1, 32, 32), 0.5)),
           dict(inpaint_images=img, inpaint_masks=torch.ones(2, 3, 32, 32)),        # a mask per channel
           dict(start_image=torch.rand(2, 3, 16, 16)),                              # start_image without start_at_stage
           dict(start_image=torch.rand(2, 3, 16, 16), start_at_stage=0),            # ... or with a stage below 1
           dict(start_at_stage=1),                                                   # the other way round
           dict(start_image=torch.rand(3, 3, 16, 16), start_at_stage=1),
           dict(start_image=torch.rand(2, 4, 16, 16), start_at_stage=1),
           dict(start_image=torch.rand(2, 3, 16, 12), start_at_stage=1),
           dict(start_image=torch.rand(2, 3, 16, 16), start_at_stage=1, stop_at_stage=1),      # start >= stop
           dict(start_image=torch.rand(2, 3, 16, 16), start_at_stage=2),            # out of range
           dict(start_image=torch.rand(2, 3, 16, 16), start_at_stage=True),
           dict(stop_at_stage=0), dict(stop_at_stage=3), dict(stop_at_stage=-1), dict(stop_at_stage=1.5)]
    for kw in bad:
        with pytest.raises(ValueError):
            im.sample(text_embeds=emb, text_masks=mask, **kw)
    with pytest.raises(TypeError):
        im.sample(emb, None, None, 1., None, False, None, img, m)          # keyword-only
    start, stop, inp, first = im._parse_inpaint(2, img, m[:, None].float(), None, None, 1)
    assert (start, stop, first) == (0, 1, None) and inp[1].dtype == torch.uint8 and inp[1].shape == (2, 32, 32) and inp[0].dtype == torch.float32
    assert im._parse_inpaint(2, None, None, None, None, None) == (0, 2, None, None)
    # a stage that takes no low-resolution image cannot start from one
    two_bases = Imagen([Unet(**TINY), Unet(**TINY)], text_encoder_name="t5_small", image_sizes=[16, 32], timesteps=25, cond_drop_prob=0.15)
    two_bases.unets[1].lowres_cond = False
    with pytest.raises(ValueError):
        two_bases.sample(text_embeds=emb, text_masks=mask, start_image=torch.rand(2, 3, 16, 16), start_at_stage=1)


# ------------------------------------------------------------------------------------------------ 3. the tails, bit exact
def _np_step(x0, sq, x, prev, z, row, history):
    """the stated order, one rounding per operation: threshold; mean = c2 x0 + c3 x; (mean += c5 prev;) x' = mean + c4 z (cN = column N)"""
    f = np.float32
    c2, c3, c4, c5 = f(row[2]), f(row[3]), f(row[4]), f(row[5])
    s = np.where(sq < f(1), f(1), sq).astype(f)[:, None]
    x0c = (np.clip(x0, -s, s) / s).astype(f)
    mean = ((c2 * x0c).astype(f) + (c3 * x).astype(f)).astype(f)
    if history:
        mean = (mean + (c5 * prev).astype(f)).astype(f)
    return (mean + (c4 * z).astype(f)).astype(f), x0c


def _np_blend(x, y, m, z, a, b, draw=True):
    """x = m ? fadd(fmul(a, y), fmul(b, z)) : x; without a draw the known pixels are y itself"""
    f = np.float32
    if not draw:
        return np.where(m, y, x)
    return np.where(m, ((f(a) * y).astype(f) + (f(b) * z).astype(f)).astype(f), x)


def _bits(t):
    return (t.cpu().numpy() if torch.is_tensor(t) else t).view(np.uint32)


def _tail_inputs(B, n, hw, S, g):
    mask = torch.zeros(B, hw, dtype=torch.uint8)
    mask[0] = (torch.rand(hw, generator=g) < 0.5).to(torch.uint8)          # a random half
    mask[1] = 1                                                             # all known; row 2: none
    known = torch.rand(B, n, generator=g) * 2 - 1
    return mask, known, torch.randn(S, B, n, generator=g)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("history", [True, False])
@pytest.mark.parametrize("n", [3 * 16 * 16, 3 * 15 * 15, 27648])
def test_inpaint_tails_bit_exact(backend, n, history):
    """mi_posterior_inpaint_fwd on injected step and known-region noise against numpy in the stated operation order, all bits of x (and of
    x0_prev); the fused forms (one workgroup per image / cooperating workgroups) give the separate kernels' bits, on injected noise and on
    Philox; a NULL inpaint block is the *_ext_fwd entry"""
    dev = setup(backend)
    lib = L.lib()
    B, T, S, hw = 3, 100, 10, n // 3
    _, tab = GaussianDiffusion(timesteps=T).sampler_tables(S, "dpmpp_2m" if history else "ddpm", known=True)
    coef = tab.to(dev).contiguous()
    g = torch.Generator().manual_seed(n + history)
    k_lo, k_hi, w = quantile_rank(n, 0.9)
    st = L.current_stream()
    dv = lambda t: t.clone().to(dev)                          # (a copy on the emulator too: the kernels update in place)
    for k, off in ((5, 0), (S - 1, 0), (3, 2), (0, 0)):
        pred2, xt = torch.randn(2 * B, n, generator=g) * 1.5, torch.randn(B, n, generator=g)
        noise, prev0 = torch.randn(S, B, n, generator=g), torch.randn(B, n, generator=g)
        mask, known, knoise = _tail_inputs(B, n, hw, S, g)
        pred2d, noised, maskd, knownd, knoised = (t.to(dev) for t in (pred2, noise, mask, known, knoise))
        tstate = torch.tensor([k + off], dtype=torch.int32, device=dev)
        x0, s_q = torch.zeros(B, n, device=dev), torch.zeros(B, device=dev)
        hist = torch.zeros(3 * B * 2 * 2048, dtype=torch.int32, device=dev)
        xa, pa = dv(xt), dv(prev0)
        cp = L.MiCfgX0Params(B, n, pred2d.data_ptr(), 1, 3.0, xa.data_ptr(), coef.data_ptr(), tstate.data_ptr(), 0, x0.data_ptr(), 0, off)
        L.check(lib.mi_cfg_x0_fwd(C.byref(cp), st))
        qp = L.MiQuantileParams(B, n, x0.data_ptr(), k_lo, k_hi, w, hist.data_ptr(), s_q.data_ptr(), None)
        L.check(lib.mi_quantile_fwd(C.byref(qp), st))
        pp = L.MiPosteriorParams(B, n, S, x0.data_ptr(), s_q.data_ptr(), xa.data_ptr(), coef.data_ptr(), tstate.data_ptr(), noised.data_ptr(), 0, 0, 0, 0, off)
        ext = lambda p: L.MiSamplerExtParams(0, p.data_ptr() if history else 0)
        ip = L.MiInpaintParams(knownd.data_ptr(), maskd.data_ptr(), hw, KNOWN_STREAM, knoised.data_ptr())
        L.check(lib.mi_posterior_inpaint_fwd(C.byref(pp), C.byref(ext(pa)), C.byref(ip), st), "mi_posterior_inpaint_fwd")
        step_x, want_prev = _np_step(x0.cpu().numpy(), s_q.cpu().numpy(), xt.numpy(), prev0.numpy(), noise[S - 1 - k].numpy(), tab[k].numpy(), history)
        m_el = np.tile(mask.numpy() != 0, (1, 3))
        want_x = _np_blend(step_x, known.numpy(), m_el, knoise[min(S - k, S - 1)].numpy(), tab[k, 6], tab[k, 7], draw=k > 0)
        assert np.array_equal(_bits(xa), _bits(want_x)), (k, off)
        assert np.array_equal(_bits(xa)[2], _bits(step_x)[2]) and not np.array_equal(_bits(xa)[0], _bits(step_x)[0])      # empty / half mask
        if k == 0:
            assert np.array_equal(_bits(xa)[1], _bits(known)[1])                   # no draw: the known pixels are y, bit for bit
        if history:
            assert np.array_equal(_bits(pa), _bits(want_prev)), (k, off)           # the thresholded x0 of every element
        # a NULL inpaint block: the *_ext_fwd entry
        xe, pe, xn, pn = dv(xt), dv(prev0), dv(xt), dv(prev0)
        pq = L.MiPosteriorParams.from_buffer_copy(pp)
        pq.x = xe.data_ptr()
        L.check(lib.mi_posterior_ext_fwd(C.byref(pq), C.byref(ext(pe)), st))
        pq.x = xn.data_ptr()
        L.check(lib.mi_posterior_inpaint_fwd(C.byref(pq), C.byref(ext(pn)), None, st))
        assert torch.equal(xe, xn) and torch.equal(pe, pn) and np.array_equal(_bits(xe), _bits(step_x))
        # the fused forms on the same inputs
        fused_null = {}
        for use_noise in (True, False):
            if not use_noise:                                  # the on-device generator: the separate kernels again, same (seed, row, stream)
                xa, pa = dv(xt), dv(prev0)
                pr = L.MiPosteriorParams(B, n, S, x0.data_ptr(), s_q.data_ptr(), xa.data_ptr(), coef.data_ptr(), tstate.data_ptr(), 0, 77, 5, 3 << 20, 0, off)
                ip = L.MiInpaintParams(knownd.data_ptr(), maskd.data_ptr(), hw, (3 << 20) | KNOWN_STREAM, 0)
                L.check(lib.mi_posterior_inpaint_fwd(C.byref(pr), C.byref(ext(pa)), C.byref(ip), st))
            for block in (ip, None):
                xs, ps_ = dv(xt), dv(prev0)
                cf = L.MiCfgX0Params(B, n, pred2d.data_ptr(), 1, 3.0, xs.data_ptr(), coef.data_ptr(), tstate.data_ptr(), 0, 0, 0, off)
                qf = L.MiQuantileParams(B, n, 0, k_lo, k_hi, w, 0, 0, 0, 0, 0)
                pf = L.MiPosteriorParams(B, n, S, 0, 0, xs.data_ptr(), coef.data_ptr(), tstate.data_ptr(), noised.data_ptr() if use_noise else 0, 77, 5, 3 << 20, 0, off)
                ef, bl = ext(ps_), (C.byref(block) if block is not None else None)
                if n <= 16384:
                    L.check(lib.mi_sampler_step_small_inpaint_fwd(C.byref(cf), C.byref(qf), C.byref(pf), C.byref(ef), bl, st), "small inpaint")
                else:
                    assert lib.mi_sampler_group_size(n) == 2
                    sync = torch.zeros(lib.mi_sampler_group_sync_bytes(B, n), dtype=torch.uint8, device=dev)
                    L.check(lib.mi_sampler_step_group_inpaint_fwd(C.byref(cf), C.byref(qf), C.byref(pf), C.byref(ef), bl, sync.data_ptr(), st), "group inpaint")
                    assert int(sync[8:12].view(torch.int32).item()) == 0
                if block is not None:
                    assert torch.equal(xs, xa) and torch.equal(ps_, pa), (k, off, use_noise)
                elif use_noise:
                    assert torch.equal(xs, xe) and torch.equal(ps_, pe), (k, off)      # NULL block: the fused *_ext_fwd result == the separate one
                    fused_null[k] = True
        assert fused_null


@pytest.mark.parametrize("backend", BACKENDS)
def test_blend0_struct_and_invalid_blocks(backend):
    dev = setup(backend)
    lib = L.lib()
    st = L.current_stream()
    assert lib.mi_struct_size(25) == C.sizeof(L.MiInpaintParams) == 48 and lib.mi_abi_version() == 12
    B, S = 3, 4
    for n in (3 * 16 * 16, 3 * 15 * 15):
        hw = n // 3
        g = torch.Generator().manual_seed(n)
        mask, known, knoise = _tail_inputs(B, n, hw, S, g)
        x = torch.randn(B, n, generator=g)
        xd, maskd, knownd, knoised = (t.clone().to(dev) for t in (x, mask, known, knoise))
        ip = L.MiInpaintParams(knownd.data_ptr(), maskd.data_ptr(), hw, KNOWN_STREAM, knoised.data_ptr())
        a, b = GaussianDiffusion(timesteps=100).known_start_coefs()
        L.check(lib.mi_inpaint_blend0_fwd(xd.data_ptr(), B, n, C.byref(ip), a, b, 77, 5, st), "mi_inpaint_blend0_fwd")
        want = _np_blend(x.numpy(), known.numpy(), np.tile(mask.numpy() != 0, (1, 3)), knoise[0].numpy(), a, b)
        assert np.array_equal(_bits(xd), _bits(want))
        # invalid blocks: hw <= 0, n % hw != 0, missing pointers -- for blend 0 and the three tails
        coef = torch.zeros(S, 8, device=dev)
        tstate = torch.zeros(1, dtype=torch.int32, device=dev)
        x0, s_q = torch.zeros(B, n, device=dev), torch.ones(B, device=dev)
        pp = L.MiPosteriorParams(B, n, S, x0.data_ptr(), s_q.data_ptr(), xd.data_ptr(), coef.data_ptr(), tstate.data_ptr(), 0, 0, 0, 0, 0, 0)
        cf = L.MiCfgX0Params(B, n, x0.data_ptr(), 0, 1.0, xd.data_ptr(), coef.data_ptr(), tstate.data_ptr(), 0, 0, 0, 0)
        qf = L.MiQuantileParams(B, n, 0, 1, 2, 0.5, 0, 0, 0, 0, 0)
        sync = torch.zeros(64, dtype=torch.uint8, device=dev)
        before = xd.clone()
        for bad in (L.MiInpaintParams(knownd.data_ptr(), maskd.data_ptr(), 0, 0, 0), L.MiInpaintParams(knownd.data_ptr(), maskd.data_ptr(), -4, 0, 0),
                    L.MiInpaintParams(knownd.data_ptr(), maskd.data_ptr(), hw - 1, 0, 0), L.MiInpaintParams(0, maskd.data_ptr(), hw, 0, 0),
                    L.MiInpaintParams(knownd.data_ptr(), 0, hw, 0, 0)):
            assert lib.mi_inpaint_blend0_fwd(xd.data_ptr(), B, n, C.byref(bad), a, b, 77, 5, st) == MI_ERR_INVALID
            assert lib.mi_posterior_inpaint_fwd(C.byref(pp), None, C.byref(bad), st) == MI_ERR_INVALID and b"inpaint" in lib.mi_last_error()
            assert lib.mi_sampler_step_small_inpaint_fwd(C.byref(cf), C.byref(qf), C.byref(pp), None, C.byref(bad), st) == MI_ERR_INVALID
            assert lib.mi_sampler_step_group_inpaint_fwd(C.byref(cf), C.byref(qf), C.byref(pp), None, C.byref(bad), sync.data_ptr(), st) == MI_ERR_INVALID
        assert torch.equal(xd, before)


# ------------------------------------------------------------------------------------------------ 4. Philox streams
@pytest.mark.parametrize("backend", BACKENDS)
def test_known_region_philox_streams(backend):
    """on-device noise: the draw of blend j for row b is mi_randn_fill on stream (stage << 20) | (3 << 18) | j with sample0 + b -- the
    keying sharding relies on.  Blend 0 with (a, b) = (0, 1) returns the draw itself; a tail with y = 0 returns c7 * draw (0 + v is exact)"""
    dev = setup(backend)
    lib = L.lib()
    st = L.current_stream()
    B, S, T, stage, seed, sample0 = 3, 10, 100, 2, 1234, 5
    _, tab = GaussianDiffusion(timesteps=T).sampler_tables(S, "ddpm", known=True)
    coef = tab.to(dev).contiguous()
    for n in (3 * 16 * 16, 3 * 15 * 15):
        hw = n // 3
        stream0 = (stage << 20) | KNOWN_STREAM
        mask = torch.ones(B, hw, dtype=torch.uint8, device=dev)
        known = torch.zeros(B, n, device=dev)
        ip = L.MiInpaintParams(known.data_ptr(), mask.data_ptr(), hw, stream0, 0)

        def draws(j):
            z = torch.zeros(B, n, device=dev)
            L.check(lib.mi_randn_fill(z.data_ptr(), B, n, seed, sample0, stream0 | j, st))
            rows = torch.zeros(B, n, device=dev)
            for b in range(B):                                    # row b of a batch == row 0 of a call that starts at sample0 + b
                L.check(lib.mi_randn_fill(rows[b].data_ptr(), 1, n, seed, sample0 + b, stream0 | j, st))
            assert torch.equal(z, rows)
            return z.cpu().numpy()

        x = torch.full((B, n), 7., device=dev)
        L.check(lib.mi_inpaint_blend0_fwd(x.data_ptr(), B, n, C.byref(ip), 0., 1., seed, sample0, st))
        assert np.array_equal(_bits(x), _bits(draws(0)))
        assert not np.array_equal(draws(0), draws(1))
        for k in (S - 1, 4, 1):
            j = S - k
            x = torch.randn(B, n).to(dev)
            x0, s_q = torch.zeros(B, n, device=dev), torch.ones(B, device=dev)
            tstate = torch.tensor([k], dtype=torch.int32, device=dev)
            pp = L.MiPosteriorParams(B, n, S, x0.data_ptr(), s_q.data_ptr(), x.data_ptr(), coef.data_ptr(), tstate.data_ptr(), 0, seed, sample0, stage << 20, 0, 0)
            L.check(lib.mi_posterior_inpaint_fwd(C.byref(pp), None, C.byref(ip), st))
            want = (np.float32(tab[k, 7]) * draws(j)).astype(np.float32)
            assert np.array_equal(x.cpu().numpy(), want), (n, k)


# ------------------------------------------------------------------------------------------------ 5. / 6. empty and full masks
def _model(backend, dev, T):
    """the two configurations of the loop tests: the 64 -> 256 golden cascade on the GPU, the tiny one-stage net at 16^2 on the emulator"""
    gpu = backend == "gpu"
    im = make_imagen([64, 256], T, dev) if gpu else tiny_imagen(16, T, dev)[0]
    return im, (256 if gpu else 16)


@pytest.mark.parametrize("backend", BACKENDS)
def test_empty_mask_is_the_plain_call(backend):
    dev = setup(backend)
    T = 25 if backend == "gpu" else 21
    im, size = _model(backend, dev, T)
    emb, mask = R.synthetic_text(2, length=16, seed=7)
    kw = dict(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., _seed=11)
    none = dict(inpaint_images=pixels(2, size, 1).to(dev), inpaint_masks=torch.zeros(2, size, size, dtype=torch.bool, device=dev))
    for solver in (dict(), dict(sampler="dpmpp_2m", sample_steps=10)):
        a = im.sample(**kw, **solver).clone()
        assert torch.equal(a, im.sample(**kw, **solver, **none)), solver
        assert a.isfinite().all() and a.std() > 0.01
    for u in im.unets:
        for ws in u.engine()._ws.values():
            keys = list(ws.sampler_state.keys())
            assert keys[0] == T and set(keys[1:]) == {(T, "inpaint"), (T, 10, "dpmpp_2m", 0.), (T, 10, "dpmpp_2m", 0., "inpaint")}
            assert len(ws.sampler_state[T].graphs) == 1 and not hasattr(ws.sampler_state[T], "ext") and ws.sampler_state[T].ip is None
            assert (ws.sampler_state[T].coef[:, 6:] == 0).all() and ws.sampler_state[(T, "inpaint")].coef[0, 6] == 1
    im.check_device_status()


@pytest.mark.parametrize("backend", BACKENDS)
def test_full_mask_returns_the_known_image(backend):
    """all True, images at the final size: normalise (2y - 1: the product is exact, one rounding) and finalise ((v + 1) * 0.5: one rounding,
    the product exact) -- three roundings of at most 2^-24 each bound the difference by 2^-22; with auto_normalize_img=False neither runs"""
    dev = setup(backend)
    T = 25 if backend == "gpu" else 21
    emb, mask = R.synthetic_text(2, length=16, seed=7)
    for normalize in (True, False):
        im, size = _model(backend, dev, T)
        im.auto_normalize_img = normalize
        y = pixels(2, size, 3) if normalize else pixels(2, size, 3, -0.1, 1.1)
        full = torch.ones(2, 1, size, size, device=dev)
        for solver in (dict(), dict(sampler="dpmpp_2m", sample_steps=10)):
            out = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., _seed=11, inpaint_images=y.to(dev), inpaint_masks=full, **solver).cpu()
            d = (out - y).abs().max().item()
            print(f"full mask, normalize={normalize}, {solver}: max|d| = {d:.3e}")
            if normalize:
                assert d <= 2. ** -22
            else:
                assert torch.equal(out, y.clamp(0., 1.))
        im.check_device_status()


# ------------------------------------------------------------------------------------------------ 7. values against the restated loop
def _values(im, sds, sizes, T, steps, sampler, eta, dev, img_size, seed, what, B=2, length=48):
    emb, mask = R.synthetic_text(B, length=length, seed=9)
    y, m = pixels(B, img_size, seed), masks_half_and_random(B, img_size, seed)
    solver = {} if steps is None else dict(sample_steps=steps, sampler=sampler, sampler_eta=eta)
    out = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., _noise=R.make_randn(21), inpaint_images=y.to(dev),
                    inpaint_masks=m.to(dev), **solver)
    ref = restated_inpaint_sample(sds, sizes, T, steps, sampler, eta, images=y, masks=m, text_embeds=emb, text_masks=mask, cond_scale=3., randn=R.make_randn(21))
    gate(out, ref, what)
    im.check_device_status()
    return out, y, m


@pytest.mark.parametrize("backend", [pytest.param("emu", marks=pytest.mark.emu)])
@pytest.mark.parametrize("sampler", ["ddpm", "dpmpp_2m"])
def test_values_emulator(backend, sampler):
    """32^2, B = 2, T = 100, S = 6, cond_scale 3, golden base weights"""
    dev = setup(backend)
    im = make_imagen([32], 100, dev)
    out, y, m = _values(im, [I.load("unet0_sd.pt")], [32], 100, 6, sampler, None, dev, 32, 5, f"emulator 32^2 T=100 S=6 {sampler} inpaint", length=16)
    keep = m[:, None].expand_as(y)
    assert (out.cpu() - y)[keep].abs().max() <= 2. ** -22 and (out.cpu() - y)[~keep].abs().max() > 0.05


@pytest.mark.parametrize("backend", GPU_ONLY)
@pytest.mark.parametrize("sampler,eta", SOLVERS)
def test_values_base_stage(backend, sampler, eta):
    """base 64^2, cond_scale 3, T = 100, S = 20, B = 2"""
    dev = setup(backend)
    im = make_imagen([64], 100, dev)
    _values(im, [I.load("unet0_sd.pt")], [64], 100, 20, sampler, eta, dev, 64, 5, f"base 64^2 T=100 S=20 {sampler} eta={eta} inpaint")


@pytest.mark.parametrize("backend", GPU_ONLY)
def test_values_default_loop(backend):
    """the default loop (the reference's table, T = 25) on the base stage, images given at 96^2 (antialiased shrink to 64)"""
    dev = setup(backend)
    im = make_imagen([64], 25, dev)
    _values(im, [I.load("unet0_sd.pt")], [64], 25, None, None, None, dev, 96, 6, "base 64^2 T=25 default loop inpaint")


@pytest.mark.parametrize("backend", GPU_ONLY)
def test_values_cascade(backend):
    """64 -> 256, T = 100, sample_steps = (25, 10), cond_scale 3, images at 256: the base stage sees the antialiased 4x shrink, the 256^2
    stage runs the grouped tail"""
    dev = setup(backend)
    im = make_imagen([64, 256], 100, dev)
    _values(im, [I.load("unet0_sd.pt"), I.load("unet1_sd.pt")], [64, 256], 100, (25, 10), "ddpm", None, dev, 256, 7, "cascade 64->256 T=100 S=(25, 10) inpaint")
    st = [v for u in im.unets for ws in u.engine()._ws.values() for v in ws.sampler_state.values()]
    assert [hasattr(v, "group_sync") for v in st] == [False, True] and all(v.ip is not None for v in st)


# ------------------------------------------------------------------------------------------------ 8. the three tail forms in the loop
@pytest.mark.parametrize("backend", BACKENDS)
def test_three_tail_forms_agree_in_the_sampling_loop(backend, monkeypatch):
    """an inpainting call ('dpmpp_2m') through the one-workgroup tail, the grouped tail and the separate kernels: identical bits"""
    from minimagen_amd import Imagen as IM
    dev = setup(backend)
    gpu = backend == "gpu"
    emb, mask = R.synthetic_text(2, length=10, seed=3)
    for S_img, kinds in ((24, ("small", "separate")), (96 if gpu else 76, ("group", "separate"))):
        outs = {}
        y, m = pixels(2, S_img + 4, 8).to(dev), masks_half_and_random(2, S_img, 8).to(dev)
        for kind in kinds:
            monkeypatch.setenv("MINIMAGEN_SAMPLER_FUSED", "0" if (kind == "separate" and S_img == 24) else "1")
            monkeypatch.setattr(IM, "SAMPLER_GROUP", 0 if kind == "separate" else 1)
            im, _ = tiny_imagen(S_img, 25, dev)
            outs[kind] = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=2., _seed=11, sample_steps=10, sampler="dpmpp_2m",
                                   inpaint_images=y, inpaint_masks=m).cpu()
            im.check_device_status()
            sts = next(iter(im.unets[0].engine()._ws.values())).sampler_state
            assert list(sts.keys()) == [(25, 10, "dpmpp_2m", 0., "inpaint")]
            assert any(hasattr(v, "group_sync") for v in sts.values()) == (kind == "group")
        a, b = (outs[k] for k in kinds)
        assert torch.equal(a, b), kinds
        assert a.isfinite().all() and a.std() > 0.01


# ------------------------------------------------------------------------------------------------ 9. sharding
@pytest.mark.parametrize("backend", BACKENDS)
def test_sharded_rows_equal_unsharded_rows(backend):
    dev = setup(backend)
    gpu = backend == "gpu"
    im = make_imagen([64], 25, dev) if gpu else tiny_imagen(16, 21, dev)[0]
    size = 64 if gpu else 16
    emb, mask = R.synthetic_text(4, length=16, seed=7)
    emb, mask = emb.to(dev), mask.to(dev)
    y, m = pixels(4, size, 9).to(dev), masks_half_and_random(4, size, 9).to(dev)
    for solver in ((dict(), dict(sampler="dpmpp_2m", sample_steps=10)) if gpu else (dict(sampler="ddpm", sample_steps=4),)):
        kw = dict(cond_scale=3., _seed=11, **solver)
        whole = im.sample(text_embeds=emb, text_masks=mask, inpaint_images=y, inpaint_masks=m, **kw).clone()
        for lo in (0, 2):
            part = im.sample(text_embeds=emb[lo:lo + 2].contiguous(), text_masks=mask[lo:lo + 2].contiguous(), inpaint_images=y[lo:lo + 2].contiguous(),
                             inpaint_masks=m[lo:lo + 2].contiguous(), _sample_offset=lo, **kw)
            assert torch.equal(part, whole[lo:lo + 2]), (solver, lo)
        assert not torch.equal(whole[:2], whole[2:])
    im.check_device_status()


# ------------------------------------------------------------------------------------------------ 10. graph reuse and bounds
@pytest.mark.parametrize("backend", BACKENDS)
def test_one_graph_serves_other_images_and_masks(backend, monkeypatch):
    from minimagen_amd import Imagen as IM
    dev = setup(backend)
    gpu = backend == "gpu"
    T, size = (25, 64) if gpu else (21, 16)          # (T = 20 has beta = 1 at the last timestep)
    new = lambda: (make_imagen([64], T, dev) if gpu else tiny_imagen(16, T, dev)[0])
    emb, mask = R.synthetic_text(2, length=16, seed=7)
    kw = dict(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., _seed=11, sample_steps=5, sampler="ddim")
    im = new()
    inputs = [dict(inpaint_images=pixels(2, size, s).to(dev), inpaint_masks=masks_half_and_random(2, size + 8 * s, s).to(dev)) for s in (1, 2)]
    outs = [im.sample(**kw, **inp).clone() for inp in inputs]
    ws = next(iter(im.unets[0].engine()._ws.values()))
    assert list(ws.sampler_state.keys()) == [(T, 5, "ddim", 0., "inpaint")] and len(ws.sampler_state[(T, 5, "ddim", 0., "inpaint")].graphs) == 1
    assert not torch.equal(outs[0], outs[1])
    for inp, out in zip(inputs, outs):
        assert torch.equal(new().sample(**kw, **inp), out)
    im.check_device_status()
    # a sweep of S with inpainting on stays within the bound on stage states
    monkeypatch.setattr(IM, "MAX_SOLVER_STATES", 2)
    im = new()
    for S in (4, 3, 2, 3):
        im.sample(**{**kw, "sample_steps": S}, **inputs[0])
        keys = [k for k in next(iter(im.unets[0].engine()._ws.values())).sampler_state if isinstance(k, tuple)]
        assert len(keys) <= 2 and keys[-1] == (T, S, "ddim", 0., "inpaint")
    im.check_device_status()


# ------------------------------------------------------------------------------------------------ 11. start / stop
@pytest.mark.parametrize("backend", GPU_ONLY)
def test_start_and_stop_at_a_stage(backend):
    dev = setup(backend)
    im = make_imagen([64, 256], 25, dev)
    emb, mask = R.synthetic_text(2, length=16, seed=7)
    kw = dict(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., _seed=11)
    whole = im.sample(**kw).clone()
    a = im.sample(**kw, stop_at_stage=1).clone()
    assert a.shape == (2, 3, 64, 64) and a.isfinite().all()
    assert torch.equal(im.sample(**kw, start_at_stage=1, start_image=a), whole)          # the noise is keyed by the stage index
    other = im.sample(**kw, start_at_stage=1, start_image=F.interpolate(a, size=(48, 48), mode='bilinear')).clone()      # through the resize
    assert other.shape == whole.shape and other.isfinite().all() and not torch.equal(other, whole)
    assert (other - whole).abs().mean() < 0.2
    im.check_device_status()


@pytest.mark.parametrize("backend", [pytest.param("emu", marks=pytest.mark.emu)])
def test_skipped_stages_launch_nothing(backend, monkeypatch):
    dev = setup(backend)
    torch.manual_seed(4)
    im = Imagen([Unet(**TINY), Unet(**TINY, lowres_cond=True)], text_encoder_name="t5_small", image_sizes=[8, 16], timesteps=21, cond_drop_prob=0.15).to(dev)
    emb, mask = R.synthetic_text(1, length=8, seed=1)
    ran, begun = [], []
    loop, begin = im._p_sample_loop, im._stage_begin
    monkeypatch.setattr(im, "_p_sample_loop", lambda unet, shape, ws, call, *a, **kw: (ran.append(call.stage), loop(unet, shape, ws, call, *a, **kw))[1])
    monkeypatch.setattr(im, "_stage_begin", lambda unet, shape, ws, call, **kw: (begun.append(call.stage), begin(unet, shape, ws, call, **kw))[1])
    kw = dict(text_embeds=emb, text_masks=mask, cond_scale=2., _seed=3, sample_steps=2)
    a = im.sample(**kw, stop_at_stage=1)
    assert a.shape == (1, 3, 8, 8) and ran == [0] and begun == [0]
    assert not im.unets[1].engine()._ws                                     # the skipped stage has not even a workspace
    del ran[:], begun[:]
    b = im.sample(**kw, start_at_stage=1, start_image=a)
    assert b.shape == (1, 3, 16, 16) and ran == [1] and begun == [1]
    assert torch.equal(b, im.sample(**kw)) and ran == [1, 0, 1]


# ------------------------------------------------------------------------------------------------ 12. forwarding
def test_forwarding_entry_points_pass_the_keywords(tmp_path):
    from PIL import Image
    from minimagen_amd import distributed, generate
    seen = []

    class Recorder:
        channels, image_sizes = 3, (8, 16)

        def sample(self, **kw):
            seen.append(kw)
            if kw.get("return_pil_images"):
                return [Image.new("RGB", (8, 8)) for _ in kw["texts"]]
            return torch.zeros(kw["text_embeds"].shape[0], 3, 8, 8)

        def parameters(self):
            return iter([torch.zeros(1)])

    y, m, s = torch.rand(3, 3, 8, 8), torch.rand(3, 8, 8) < 0.5, torch.rand(3, 3, 4, 4)
    args = dict(inpaint_images=y[:2], inpaint_masks=m[:2], start_image=s[:2], start_at_stage=1, stop_at_stage=2)
    generate.sample_and_save(["a", "b"], minimagen=Recorder(), sample_args=dict(cond_scale=3., **args), save_directory=str(tmp_path / "out"))
    assert all(seen[-1][k] is v for k, v in args.items()) and seen[-1]["cond_scale"] == 3.
    # the technique of the existing forwarding test, for both ranks of a world of 2: rank r gets rows shard_bounds(3, 2, r) of the three tensors
    for rank in (0, 1):
        lo, hi = distributed.shard_bounds(3, 2, rank)
        import unittest.mock as mock
        with mock.patch.object(distributed.dist, "is_initialized", lambda: True), mock.patch.object(distributed.dist, "get_world_size", lambda g=None: 2), \
                mock.patch.object(distributed.dist, "get_rank", lambda g=None: rank):
            out = distributed.sample_distributed(Recorder(), text_embeds=torch.zeros(3, 4, 16), gather=False, inpaint_images=y, inpaint_masks=m,
                                                 start_image=s, start_at_stage=1, stop_at_stage=2)
        kw = seen[-1]
        assert out.shape[0] == hi - lo and kw["_sample_offset"] == lo and kw["start_at_stage"] == 1 and kw["stop_at_stage"] == 2
        assert torch.equal(kw["inpaint_images"], y[lo:hi]) and torch.equal(kw["inpaint_masks"], m[lo:hi]) and torch.equal(kw["start_image"], s[lo:hi])
        assert kw["text_embeds"].shape[0] == hi - lo
    for fn in (generate.sample_and_save, distributed.sample_distributed):
        assert "inpaint_images" in fn.__doc__ and "start_image" in fn.__doc__
