"""Imagen.sample(init_images=, init_strength=): starting the sampling loop from a noised image of the caller's (SDEdit; DESIGN.md section
25).  The start step and level and the 'dpmpp_2m' table with a start (host, fp64 identities), argument validation and forwarding (host),
the one new launch mi_init_noise_fwd bit for bit against numpy, the loop against a restated loop on injected noise (the project's gate,
SURVEY.md 8(c): max|d| < 1e-4 and mean|d| < 1e-5 on [0, 1] images) and the invariants of the loop (graphs, sharding, the untouched
default call, stages, inpainting, guidance plans)."""
import dataclasses
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from minimagen_amd import _lib as L
from minimagen_amd import sampler as S
from minimagen_amd.Imagen import Imagen
from minimagen_amd.Unet import Unet
from minimagen_amd.diffusion_model import GaussianDiffusion
from oracle import resize_restated
from oracle import restated as R
from tests import _inputs as I
from tests._backend import BACKENDS, GPU_ONLY, setup
from tests.test_sample_steps import SOLVERS, TINY, gate, make_imagen, tiny_imagen


def pixels(B, size, seed, lo=0., hi=1.):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, 3, size, size, generator=g) * (hi - lo) + lo


def abar64(T):
    betas = np.linspace(1000 / T * 1e-4, 1000 / T * 0.02, T, dtype=np.float64)
    return np.cumprod(1. - betas)


def level(T, steps, a0):
    """(fp32(sqrt(abar_tau)), fp32(sqrt(1 - abar_tau))) at tau = tau_{S-1-a0}, recomputed here in fp64 from the betas"""
    S_ = T if steps is None else steps
    tau = list(range(T)) if steps is None else [(2 * k * (T - 1) + (S_ - 1)) // (2 * (S_ - 1)) for k in range(S_)]
    a = abar64(T)[tau[S_ - 1 - a0]]
    return float(np.float32(math.sqrt(a))), float(np.float32(math.sqrt(1. - a)))


def start_step(S_, s):
    return S_ - min(S_, max(1, math.floor(s * S_ + 0.5)))


def tiny_cascade(T, dev, seed=4):
    """16 -> 32, two tiny U-Nets -> (Imagen, their state dicts)"""
    torch.manual_seed(seed)
    im = Imagen([Unet(**TINY), Unet(**TINY, lowres_cond=True)], text_encoder_name="t5_small", image_sizes=[16, 32], timesteps=T, cond_drop_prob=0.15)
    sds = [{k: v.clone() for k, v in u.state_dict().items()} for u in im.unets]
    return im.to(dev), sds


def restated_init_sample(sds, sizes, T, steps, sampler, eta, *, init, strengths, text_embeds, text_masks, cond_scale=1., scales=None, images=None,
                         masks=None, randn, lowres_sample_noise_level=0.2):
    """tests.test_sample_steps.restated_sample started from an image: per stage the draw order is low-resolution noise, x_T, the S step draws
    and (inpainting) the S known-region draws, whatever is skipped; a stage with a strength starts at x = a y' + b x_T and walks the rows
    S-1-a0 .. 0 of the table built with ``start`` = a0, step draw zs[S-1-k].  ``steps`` per stage: an int or None (the default loop on
    sampler_coef_table).  ``scales`` (per stage None or [S], execution order of the FULL loop): the guidance scale of the step, one forward
    where it is 1.  ``images`` / ``masks``: inpainting, blend 0 at the starting level with the known-region draw a0."""
    b = text_embeds.shape[0]
    lowres_sched = R.Schedule(T)
    gd = GaussianDiffusion(timesteps=T)
    known = images is not None
    img = None
    for stage, (sd, size, S_, strength) in enumerate(zip(sds, sizes, steps, strengths)):
        kw = {}
        if "to_lowres_time_hiddens.1.weight" in sd:
            lt = lowres_sched.get_times(b, lowres_sample_noise_level)
            low = resize_restated.resize(img, scale_factors=size / img.shape[-1], pad_mode='reflect') if img.shape[-1] != size else img
            low = lowres_sched.q_sample(low, int(lt[0]), randn(low.shape))
            kw.update(lowres_cond_img=low * 2 - 1, lowres_noise_times=lt)
        a0 = 0 if strength is None else start_step(T if S_ is None else S_, strength)
        if S_ is None:
            n_steps, tau, tab = T, torch.arange(T), gd.sampler_coef_table(known=known)
        else:
            n_steps = S_
            tau, tab = gd.sampler_tables(S_, sampler, eta, known=known, start=a0)
        at = lambda t: (resize_restated.resize(t, scale_factors=size / t.shape[-1], pad_mode='reflect') if t.shape[-1] != size else t).clamp(0., 1.) * 2 - 1
        shape = (b, 3, size, size)
        x, prev = randn(shape), torch.zeros(shape)
        zs = [randn(shape) for _ in range(n_steps)]
        ks = [randn(shape) for _ in range(n_steps)] if known else None
        la, lb = level(T, S_, a0)
        if strength is not None:
            x = la * at(init) + lb * x
        if known:
            y = at(images)
            m = F.interpolate(masks.float()[:, None], size=(size, size), mode='nearest') != 0
            x = torch.where(m, la * y + lb * ks[a0], x)
        w = None if (scales is None or scales[stage] is None) else torch.as_tensor(scales[stage], dtype=torch.float32)
        for k in range(n_steps - 1 - a0, -1, -1):
            t = torch.full((b,), int(tau[k]), dtype=torch.long)
            if w is None:
                pred = R.unet_forward_with_cond_scale(sd, x, t, text_embeds=text_embeds, text_mask=text_masks, cond_scale=cond_scale, **kw)
            else:
                pred = R.unet_forward(sd, x, t, text_embeds=text_embeds, text_mask=text_masks, cond_drop_prob=0., **kw)
                if w[n_steps - 1 - k] != 1.:
                    neg = R.unet_forward(sd, x, t, text_embeds=text_embeds, text_mask=text_masks, cond_drop_prob=1., **kw)
                    pred = neg + (pred - neg) * w[n_steps - 1 - k]
            x0 = tab[k, 0] * x - tab[k, 1] * pred
            s, *_ = R.dynamic_threshold_quantile(x0.reshape(b, -1).abs(), 0.9)
            s = s.clamp(min=1.).reshape(b, 1, 1, 1)
            x0 = x0.clamp(-s, s) / s
            x = ((tab[k, 2] * x0 + tab[k, 3] * x) + tab[k, 5] * prev) + tab[k, 4] * zs[n_steps - 1 - k]
            prev = x0
            if known:
                x = torch.where(m, tab[k, 6] * y + tab[k, 7] * ks[n_steps - k] if k > 0 else y, x)
        img = (x.clamp(-1., 1.) + 1) * 0.5
    return img


# ------------------------------------------------------------------------------------------------ 1. start step and level (host)
def test_start_step_and_level():
    for S_ in (2, 10, 25):
        for s in (1e-6, 0.04, 0.05, 0.5, 0.96, 1.0):
            a0 = S.init_start_step(S_, s)
            m = min(S_, max(1, math.floor(s * S_ + 0.5)))
            assert a0 == S_ - m and 1 <= S_ - a0 <= S_, (S_, s, a0)
    assert S.init_start_step(10, 1.) == 0 and S.init_start_step(10, 1e-6) == 9 and S.init_start_step(10, 0.5) == 5 and S.init_start_step(10, 0.04) == 9
    assert S.init_start_step(25, 0.5) == 12 and S.init_start_step(2, 0.5) == 1 and S.init_start_step(25, 0.96) == 1
    for bad in (0., -0.5, 1.5, True, float("nan"), "0.5", None):
        with pytest.raises(ValueError):
            S.init_start_step(10, bad)
    for T in (25, 100, 1000):
        gd = GaussianDiffusion(timesteps=T)
        assert gd.init_start_coefs() == gd.init_start_coefs(None, 0) == gd.init_start_coefs(10, 0) == gd.known_start_coefs()
        for steps in (None, 10):
            S_ = T if steps is None else steps
            tab = gd.sampler_coef_table(known=True) if steps is None else gd.sampler_tables(steps, "ddpm", known=True)[1]
            for start in sorted({0, 1, 2, S_ // 2, S_ - 2, S_ - 1}):
                got = gd.init_start_coefs(steps, start)
                assert got == level(T, steps, start), (T, steps, start)
                assert all(isinstance(v, float) for v in got) and abs(got[0] ** 2 + got[1] ** 2 - 1) < 1e-6
                if start >= 1:                    # the level behind step S - start: columns 6 and 7 of that row, bit for bit
                    assert got == (float(tab[S_ - start, 6]), float(tab[S_ - start, 7])), (T, steps, start)
            for bad in (-1, S_, True, 1.5):
                with pytest.raises(ValueError):
                    gd.init_start_coefs(steps, bad)


# ------------------------------------------------------------------------------------------------ 2. dpmpp_2m with a start (host)
def test_dpmpp_2m_with_a_start():
    """the first EXECUTED step has no history: its row is the first-order step (= DDIM, as test_first_dpmpp_step_is_ddim asserts for the
    first row of the full loop); nothing else moves, for any sampler"""
    gd = GaussianDiffusion(timesteps=100)
    for S_ in (4, 10, 37):
        _, _, dd = gd._sampler_tables64(S_, "ddim", None)
        tau0, a, dp0 = gd._sampler_tables64(S_, "dpmpp_2m", None)
        assert torch.equal(gd._sampler_tables64(S_, "dpmpp_2m", None, start=0)[2], dp0)
        ap = torch.cat([torch.ones(1, dtype=torch.float64), a[:-1]])
        for start in range(1, S_ - 1):
            tau, a1, dp = gd._sampler_tables64(S_, "dpmpp_2m", None, start=start)
            k = S_ - 1 - start
            assert torch.equal(tau, tau0) and torch.equal(a1, a)
            assert (dp[k] - dd[k]).abs().max() < 1e-13 and dp[k, 5] == 0
            assert (dp0[k, 2] - dp[k, 2]).abs() > 1e-4                    # ... and it was second order before
            others = [r for r in range(S_) if r != k]
            assert torch.equal(dp[others], dp0[others])
            assert abs(dp[k, 3] * a[k].sqrt() + dp[k, 2] + dp[k, 5] - ap[k].sqrt()) < 1e-13
            t32 = gd.sampler_tables(S_, "dpmpp_2m", start=start)[1]
            assert torch.equal(t32, dp.to(torch.float32))
            for sampler, eta in (("ddpm", None), ("ddim", None), ("ddim", 0.5)):
                assert torch.equal(gd._sampler_tables64(S_, sampler, eta, start=start)[2], gd._sampler_tables64(S_, sampler, eta)[2])
        for start in (S_ - 1,):                                            # only the last step runs: row 0 returns x0, as ever
            assert torch.equal(gd._sampler_tables64(S_, "dpmpp_2m", None, start=start)[2], dp0)
        known = gd._sampler_tables64(S_, "dpmpp_2m", None, known=True, start=1)[2]
        assert torch.equal(known[:, :6], gd._sampler_tables64(S_, "dpmpp_2m", None, start=1)[2][:, :6]) and known[0, 6] == 1
        for bad in (-1, S_, True):
            with pytest.raises(ValueError):
                gd.sampler_tables(S_, "dpmpp_2m", start=bad)


# ------------------------------------------------------------------------------------------------ 3. argument validation (host)
def test_argument_validation():
    """bad or inconsistent values raise ValueError before anything is launched (no backend is loaded here: a launch would need one)"""
    im = Imagen([Unet(**TINY), Unet(**TINY, lowres_cond=True)], text_encoder_name="t5_small", image_sizes=[16, 32], timesteps=25, cond_drop_prob=0.15)
    emb, mask = R.synthetic_text(2, length=8, seed=1)
    img = torch.rand(2, 3, 32, 32)
    bad = [dict(init_images=img),                                                       # one keyword without the other
           dict(init_strength=0.5),
           dict(init_images=torch.rand(3, 3, 32, 32), init_strength=0.5),               # batch != text batch
           dict(init_images=torch.rand(2, 4, 32, 32), init_strength=0.5),               # channel count
           dict(init_images=torch.rand(2, 3, 32, 24), init_strength=0.5),               # not square
           dict(init_images=torch.rand(2, 3, 32), init_strength=0.5),
           dict(init_images=(img * 255).to(torch.uint8), init_strength=0.5),            # not float
           dict(init_images=img.tolist(), init_strength=0.5),
           dict(init_images=img, init_strength=0.), dict(init_images=img, init_strength=-0.1), dict(init_images=img, init_strength=1.5),
           dict(init_images=img, init_strength=True), dict(init_images=img, init_strength=float("nan")), dict(init_images=img, init_strength="0.5"),
           dict(init_images=img, init_strength=[0.5]), dict(init_images=img, init_strength=[0.5] * 3),      # one entry per stage
           dict(init_images=img, init_strength=[0.5, 0.]), dict(init_images=img, init_strength=[True, 0.5]),
           dict(init_images=img, init_strength=[None, float("nan")]),
           dict(init_images=img, init_strength=[None, None]),                           # None for every stage
           dict(init_images=img, init_strength=[None, 0.5], stop_at_stage=1),           # ... for every stage that RUNS
           dict(init_images=img, init_strength=[0.5, None], start_image=torch.rand(2, 3, 16, 16), start_at_stage=1)]
    for kw in bad:
        with pytest.raises(ValueError):
            im.sample(text_embeds=emb, text_masks=mask, **kw)
    with pytest.raises(TypeError):
        im.sample(emb, None, None, 1., None, False, None, img, 0.5)          # keyword-only
    solvers = im._parse_solver((None, 10), "ddim", None)
    assert im._parse_init(2, None, None, solvers, 0, 2) == (None, [None, None])
    y, starts = im._parse_init(2, img.double(), 0.5, solvers, 0, 2)
    assert y.dtype == torch.float32 and starts == [S.init_start_step(25, 0.5), S.init_start_step(10, 0.5)] == [12, 5]
    assert im._parse_init(2, img, [None, 1.], solvers, 0, 2)[1] == [None, 0]
    # a strength for a stage that start_at_stage / stop_at_stage excludes is ignored
    assert im._parse_init(2, img, [0.5, 0.25], solvers, 0, 1)[1] == [12, None]
    assert im._parse_init(2, img, (0.5, 0.25), solvers, 1, 2)[1] == [None, 7]


# ------------------------------------------------------------------------------------------------ 4. forwarding (host)
def test_forwarding_entry_points_pass_the_keywords(tmp_path):
    """generate.sample_and_save(sample_args=) and distributed.sample_distributed(**kwargs) hand the two keywords to Imagen.sample (a recording
    stand-in for the model), init_images sharded by the captions' row bounds, and say so"""
    import unittest.mock as mock
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

    y = torch.rand(3, 3, 8, 8)
    args = dict(init_images=y[:2], init_strength=[0.5, None])
    generate.sample_and_save(["a", "b"], minimagen=Recorder(), sample_args=dict(cond_scale=3., **args), save_directory=str(tmp_path / "out"))
    assert all(seen[-1][k] is v for k, v in args.items()) and seen[-1]["cond_scale"] == 3.
    out = distributed.sample_distributed(Recorder(), text_embeds=torch.zeros(3, 4, 16), init_images=y, init_strength=0.75)
    assert out.shape[0] == 3 and torch.equal(seen[-1]["init_images"], y) and seen[-1]["init_strength"] == 0.75 and seen[-1]["_sample_offset"] == 0
    for rank in (0, 1):
        lo, hi = distributed.shard_bounds(3, 2, rank)
        with mock.patch.object(distributed.dist, "is_initialized", lambda: True), mock.patch.object(distributed.dist, "get_world_size", lambda g=None: 2), \
                mock.patch.object(distributed.dist, "get_rank", lambda g=None: rank):
            out = distributed.sample_distributed(Recorder(), text_embeds=torch.zeros(3, 4, 16), gather=False, init_images=y, init_strength=[0.5, 0.25])
        kw = seen[-1]
        assert out.shape[0] == hi - lo and kw["_sample_offset"] == lo and kw["init_strength"] == [0.5, 0.25]
        assert torch.equal(kw["init_images"], y[lo:hi]) and kw["init_images"].is_contiguous() and kw["text_embeds"].shape[0] == hi - lo
    for fn in (generate.sample_and_save, distributed.sample_distributed):
        assert "init_images" in fn.__doc__ and "init_strength" in fn.__doc__
    assert "init_images" in Imagen.sample.__doc__ and "init_strength" in Imagen.sample.__doc__


# ------------------------------------------------------------------------------------------------ 5. the launch, bit for bit
def _bits(t):
    return (t.cpu().numpy() if torch.is_tensor(t) else t).view(np.uint32)


def _np_init_noise(img, z, a, b, normalize):
    """the stated order, one rounding per operation: clamp; *2 then -1; a y'; b z; their sum"""
    f = np.float32
    y = np.clip(img, f(0), f(1)).astype(f)
    if normalize:
        y = ((y * f(2)).astype(f) - f(1)).astype(f)
    return ((f(a) * y).astype(f) + (f(b) * z).astype(f)).astype(f)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("n", [3 * 16 * 16, 3 * 5 * 5, 8])
def test_init_noise_kernel_bit_exact(backend, n):
    """16-byte accesses (n % 4 == 0, aligned), element by element (n % 4 != 0; and n % 4 == 0 behind a pointer 4 bytes off alignment), one
    partial quad per row at n = 75, several rows; Philox == mi_randn_fill of the same (seed, sample0, stream) == the injected form; rows of
    a sample0 = 5 call are rows 5 .. of a sample0 = 0 call"""
    dev = setup(backend)
    lib, st = L.lib(), L.current_stream()
    B, seed, stream_id = 3, 1234, (2 << 20) | (1 << 19) | 1
    gd = GaussianDiffusion(timesteps=100)
    g = torch.Generator().manual_seed(n)
    img = (torch.rand(B + 5, n, generator=g) * 1.4 - 0.2)                 # values below 0 and above 1: the clamp
    img[0, :3] = torch.tensor([-0.5, 1.5, 0.25])
    assert (img < 0).any() and (img > 1).any()
    imgd = img.to(dev).contiguous()

    def run(rows, sample0, a, b, normalize, noise=None, shift=0):
        nb = len(rows)
        buf = torch.full((nb * n + 4,), 7., device=dev)
        x = buf[shift:shift + nb * n]
        src = imgd[rows].contiguous()
        L.check(lib.mi_init_noise_fwd(src.data_ptr(), x.data_ptr(), nb, n, normalize, a, b, seed, sample0, stream_id, L.ptr(noise), st), "mi_init_noise_fwd")
        if backend == "gpu":
            torch.cuda.synchronize()
        assert (buf[:shift] == 7.).all() and (buf[shift + nb * n:] == 7.).all()          # nothing outside the rows is written
        return x.reshape(nb, n).cpu().numpy()

    def fill(nb, sample0):
        z = torch.zeros(nb, n, device=dev)
        L.check(lib.mi_randn_fill(z.data_ptr(), nb, n, seed, sample0, stream_id, st), "mi_randn_fill")
        return z

    z0, z5 = fill(B + 5, 0), fill(B, 5)
    assert torch.equal(z0[5:], z5)
    for start in (3, 7):
        a, b = gd.init_start_coefs(10, start)
        assert 0 < a < 1 and 0 < b < 1
        for normalize in (0, 1):
            want = _np_init_noise(img[:B].numpy(), z0[:B].cpu().numpy(), a, b, normalize)
            got = run(list(range(B)), 0, a, b, normalize)
            assert np.array_equal(_bits(got), _bits(want)), (start, normalize)
            assert np.array_equal(_bits(run(list(range(B)), 0, a, b, normalize, noise=z0[:B].contiguous())), _bits(want))       # the injected form
            assert np.array_equal(_bits(run(list(range(B)), 0, a, b, normalize, shift=1)), _bits(want))                      # off alignment
            assert np.array_equal(_bits(run(list(range(B)), 0, a, b, normalize, noise=z0.reshape(-1)[1:1 + B * n], shift=1)),
                                  _bits(_np_init_noise(img[:B].numpy(), z0.reshape(-1)[1:1 + B * n].reshape(B, n).cpu().numpy(), a, b, normalize)))
            # sharding: rows 5 .. of a sample0 = 0 call
            whole = run(list(range(B + 5)), 0, a, b, normalize)
            part = run(list(range(5, B + 5)), 5, a, b, normalize)
            assert np.array_equal(_bits(part), _bits(whole[5:])) and not np.array_equal(part, whole[:B])
    # (0, 1): the x_T draw itself (the level of T = 20, where abar_{T-1} is exactly 0)
    assert np.array_equal(_bits(run(list(range(B)), 0, 0., 1., 1)), _bits(z0[:B]))
    # NaN pixels stay NaN (torch.clamp), bad arguments are refused
    nan_img = imgd[:1].clone()
    nan_img[0, 1] = float("nan")
    x = torch.zeros(1, n, device=dev)
    L.check(lib.mi_init_noise_fwd(nan_img.data_ptr(), x.data_ptr(), 1, n, 1, 0.5, 0.5, seed, 0, stream_id, 0, st))
    assert x[0, 1].isnan() and x.isnan().sum() == 1
    for args in ((0, x.data_ptr(), 1, n), (nan_img.data_ptr(), 0, 1, n), (nan_img.data_ptr(), x.data_ptr(), 0, n), (nan_img.data_ptr(), x.data_ptr(), 1, 0)):
        assert lib.mi_init_noise_fwd(*args, 1, 0.5, 0.5, seed, 0, stream_id, 0, st) == -1
    assert lib.mi_abi_version() == 12 and lib.mi_struct_size(35) == -1


# ------------------------------------------------------------------------------------------------ 6. values against the restated loop
def _captions(B=2, length=16, seed=7):
    return R.synthetic_text(B, length=length, seed=seed)


@functools.lru_cache(maxsize=None)
def _golden_reference(sampler, eta):
    emb, mask = _captions()
    return restated_init_sample([I.load("unet0_sd.pt")], [32], 100, (6,), sampler, eta, init=pixels(2, 48, 5), strengths=(0.5,), text_embeds=emb,
                                text_masks=mask, cond_scale=3., randn=R.make_randn(3))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("sampler,eta", SOLVERS)
def test_values_one_stage(backend, sampler, eta):
    """32^2, golden base weights, B = 2, T = 100, S = 6, cond_scale 3, strength 0.5 (a0 = 3: tau = 40, 20, 0), the init image at 48^2
    (antialiased shrink)"""
    dev = setup(backend)
    im = make_imagen([32], 100, dev)
    emb, mask = _captions()
    out = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., _noise=R.make_randn(3), sample_steps=6, sampler=sampler, sampler_eta=eta,
                    init_images=pixels(2, 48, 5).to(dev), init_strength=0.5)
    im.check_device_status()
    gate(out, _golden_reference(sampler, eta), f"32^2 T=100 S=6 {sampler} eta={eta} init 0.5")
    keys = list(next(iter(im.unets[0].engine()._ws.values())).sampler_state.keys())
    assert keys == [(100, 6, sampler, {"ddpm": 1., "dpmpp_2m": 0.}.get(sampler, eta or 0.)) + ((("start", 3),) if sampler == "dpmpp_2m" else ())]


@functools.lru_cache(maxsize=None)
def _cascade_reference(sampler):
    _, sds = tiny_cascade(25, torch.device("cpu"))
    emb, mask = _captions()
    run = lambda strengths: restated_init_sample(sds, [16, 32], 25, (5, 5), sampler, None, init=pixels(2, 32, 6), strengths=strengths, text_embeds=emb,
                                                 text_masks=mask, cond_scale=3., randn=R.make_randn(8))
    return run((0.5, 0.4)), run((None, None))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("sampler", ["ddpm", "dpmpp_2m"])
def test_values_cascade_tiny(backend, sampler):
    """16 -> 32 tiny, B = 2, T = 25, S = (5, 5), strengths [0.5, 0.4]: m = (3, 2) -- and that loop really differs from the loop from pure noise"""
    dev = setup(backend)
    im, _ = tiny_cascade(25, dev)
    emb, mask = _captions()
    out = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., _noise=R.make_randn(8), sample_steps=5, sampler=sampler,
                    init_images=pixels(2, 32, 6).to(dev), init_strength=[0.5, 0.4])
    im.check_device_status()
    ref, plain = _cascade_reference(sampler)
    assert (ref - plain).abs().max() >= 1e-2
    gate(out, ref, f"16->32 tiny T=25 S=(5, 5) {sampler} init [0.5, 0.4]")


# ------------------------------------------------------------------------------------------------ 7. one step only
@pytest.mark.parametrize("backend", BACKENDS)
def test_one_step_only(backend):
    """a strength so small that m = 1: the default loop (a0 = 24, row 0 of the reference's table) and 'dpmpp_2m' at S = 5 (a0 = 4)"""
    dev = setup(backend)
    im, sd = tiny_imagen(16, 25, dev)
    emb, mask = _captions()
    y = pixels(2, 16, 2)
    for solver, steps, sampler in ((dict(), None, "ddpm"), (dict(sample_steps=5, sampler="dpmpp_2m"), 5, "dpmpp_2m")):
        out = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., _noise=R.make_randn(4), init_images=y.to(dev), init_strength=1e-6, **solver)
        ref = restated_init_sample([sd], [16], 25, (steps,), sampler, None, init=y, strengths=(1e-6,), text_embeds=emb, text_masks=mask, cond_scale=3.,
                                   randn=R.make_randn(4))
        gate(out, ref, f"16^2 T=25 one step {solver}")
        assert (out.cpu() - y).abs().mean() < 0.25          # one step from abar_0: near the image
    im.check_device_status()


# ------------------------------------------------------------------------------------------------ 8. full strength at T = 20
@pytest.mark.parametrize("backend", BACKENDS)
def test_full_strength_at_T20_is_the_plain_call(backend):
    """at T = 20 abar_{T-1} is exactly 0: the level of x_T is (0, 1), x = 0 y' + 1 eps = eps, and the call IS the plain one -- same states, same
    graphs, same bits.  The same abar = 0 makes column 0 of the first step's row sqrt(1 / 0) = inf, so the plain call's images at T = 20 are
    NaN, with or without the keywords (why the other tests avoid T = 20): the images are compared as bit patterns, which is what torch.equal
    asks of finite values, and the starting point itself -- finite -- with torch.equal on the stage's x right behind stage_begin."""
    dev = setup(backend)
    gd = GaussianDiffusion(timesteps=20)
    assert gd.known_start_coefs() == (0., 1.) == gd.init_start_coefs(None, 0) == gd.init_start_coefs(7, 0)
    im, _ = tiny_imagen(16, 20, dev)
    emb, mask = _captions()
    kw = dict(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., _seed=11)
    y = pixels(2, 24, 3).to(dev)
    for solver in (dict(), dict(sampler="ddim", sample_steps=7)):
        a = im.sample(**kw, **solver).clone()
        b = im.sample(**kw, **solver, init_images=y, init_strength=1.)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), solver
    ws = next(iter(im.unets[0].engine()._ws.values()))
    assert list(ws.sampler_state.keys()) == [20, (20, 7, "ddim", 0.)] and all(len(v.graphs) == 1 for v in ws.sampler_state.values())
    for solver in (None, (7, "ddim", 0.)):
        begin = dict(noise_scheduler=im.noise_schedulers[0], noise=S.Noise(seed=11, sample0=0))
        plain = S.StageCall(0, 20 if solver is None else solver[0], solver)
        S.stage_begin(im.unets[0], (2, 3, 16, 16), ws, plain, **begin)
        x_t = ws.x.clone()
        S.stage_begin(im.unets[0], (2, 3, 16, 16), ws, dataclasses.replace(plain, start=0, init=(y, True)), **begin)
        assert torch.equal(ws.x, x_t) and x_t.isfinite().all() and x_t.std() > 0.5, solver
    im.check_device_status()


# ------------------------------------------------------------------------------------------------ 9. invariants
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("sampler", ["ddpm", "dpmpp_2m"])
def test_loop_invariants(backend, sampler):
    """(a) graph == eager for m = 5 (one graph of five steps) and m = 7 (five + two); (b) another init image replays the same graphs;
    (c) sharded rows == unsharded rows; (d) the plain call before and after an init call gives the same bits"""
    dev = setup(backend)
    im, _ = tiny_imagen(16, 25, dev)
    emb, mask = _captions(4)
    emb, mask = emb.to(dev), mask.to(dev)
    y = pixels(4, 16, 1).to(dev)
    two = dict(text_embeds=emb[:2].contiguous(), text_masks=mask[:2].contiguous(), cond_scale=3., _seed=11, sample_steps=10, sampler=sampler)
    plain = im.sample(**two).clone()
    outs = {}
    for s, m in ((0.5, 5), (0.7, 7)):
        assert 10 - S.init_start_step(10, s) == m
        a = outs[m] = im.sample(**two, init_images=y[:2].contiguous(), init_strength=s).clone()
        assert torch.equal(a, im.sample(**two, init_images=y[:2].contiguous(), init_strength=s, _use_graph=False)), m
        assert a.isfinite().all() and a.min() >= 0. and a.max() <= 1. and a.std() > 0.01
    assert not torch.equal(outs[5], outs[7]) and not torch.equal(outs[5], plain)
    sts = next(iter(im.unets[0].engine()._ws.values())).sampler_state
    count = lambda: {k: sorted(e["per"] for e in v.graphs.values()) for k, v in sts.items()}
    base = (25, 10, sampler, 1. if sampler == "ddpm" else 0.)
    if sampler == "ddpm":
        assert count() == {base: [2, 5, 5]}                                      # the full loop's graph, and the lengths 5 and 2 of the runs
    else:
        assert count() == {base: [5], base + (("start", 5),): [5], base + (("start", 3),): [2, 5]}
    before = count()
    other = im.sample(**two, init_images=y[2:].contiguous(), init_strength=0.5)          # (b)
    assert count() == before and not torch.equal(other, outs[5])
    assert torch.equal(im.sample(**two), plain)                                  # (d)
    assert torch.equal(im.sample(**two, init_images=y[:2].contiguous(), init_strength=0.5), outs[5])
    whole = im.sample(text_embeds=emb, text_masks=mask, cond_scale=3., _seed=11, sample_steps=10, sampler=sampler, init_images=y, init_strength=0.5)      # (c)
    assert torch.equal(whole[:2], outs[5])
    part = im.sample(text_embeds=emb[2:].contiguous(), text_masks=mask[2:].contiguous(), cond_scale=3., _seed=11, sample_steps=10, sampler=sampler,
                     init_images=y[2:].contiguous(), init_strength=0.5, _sample_offset=2)
    assert torch.equal(part, whole[2:]) and not torch.equal(part, other)
    im.check_device_status()


@pytest.mark.parametrize("backend", BACKENDS)
def test_stages_with_and_without_a_strength(backend):
    """(e) [None, s]: the base stage is the plain call's -- its second stage, started from the PLAIN call's stage-0 image, reproduces it; (f) [s, None]: the second stage, started from that call's stage-0 image, reproduces
    the cascade (the noise is keyed by the stage index)"""
    dev = setup(backend)
    im, _ = tiny_cascade(25, dev)
    emb, mask = _captions()
    kw = dict(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., _seed=11, sample_steps=4)
    y = pixels(2, 32, 9).to(dev)
    base = im.sample(**kw, stop_at_stage=1).clone()
    with pytest.raises(ValueError):                  # ([None, s] with stop_at_stage=1: None for every stage that runs -- rejected, so (e) goes through start_image)
        im.sample(**kw, stop_at_stage=1, init_images=y, init_strength=[None, 0.5])
    whole = im.sample(**kw).clone()
    late = im.sample(**kw, init_images=y, init_strength=[None, 0.5]).clone()
    assert not torch.equal(late, whole)
    assert torch.equal(im.sample(**kw, init_images=y, init_strength=[None, 0.5], start_at_stage=1, start_image=base), late)
    early = im.sample(**kw, init_images=y, init_strength=[0.5, None]).clone()
    stage0 = im.sample(**kw, init_images=y, init_strength=[0.5, None], stop_at_stage=1).clone()
    assert not torch.equal(stage0, base) and not torch.equal(early, whole)
    assert torch.equal(im.sample(**kw, start_at_stage=1, start_image=stage0), early)                                  # (f)
    im.check_device_status()


# ------------------------------------------------------------------------------------------------ 10. with inpainting
@pytest.mark.parametrize("backend", BACKENDS)
def test_with_inpainting(backend):
    """full mask: the known image (normalise, blend, finalise: three roundings of at most 2^-24 each, as test_inpaint's bound; without
    auto_normalize_img none of them, bit for bit); empty mask: the bits of the init-only call; half mask: the restated loop, blend 0 at the
    starting level with the known-region draw a0"""
    dev = setup(backend)
    emb, mask = _captions()
    init, y = pixels(2, 16, 1), pixels(2, 16, 3)
    text = dict(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3.)
    solver = dict(sample_steps=5, sampler="dpmpp_2m")
    start = dict(init_images=init.to(dev), init_strength=0.6)
    assert S.init_start_step(5, 0.6) == 2
    for normalize in (True, False):
        im, sd = tiny_imagen(16, 25, dev)
        im.auto_normalize_img = normalize
        yk = y if normalize else pixels(2, 16, 3, -0.1, 1.1)
        full = im.sample(**text, _seed=11, **solver, **start, inpaint_images=yk.to(dev), inpaint_masks=torch.ones(2, 16, 16, dtype=torch.bool, device=dev)).cpu()
        if normalize:
            assert (full - yk).abs().max() <= 2. ** -22
        else:
            assert torch.equal(full, yk.clamp(0., 1.))
    im, sd = tiny_imagen(16, 25, dev)
    only = im.sample(**text, _seed=11, **solver, **start).clone()
    empty = im.sample(**text, _seed=11, **solver, **start, inpaint_images=y.to(dev), inpaint_masks=torch.zeros(2, 16, 16, dtype=torch.bool, device=dev))
    assert torch.equal(empty, only)
    half = torch.rand(2, 16, 16, generator=torch.Generator().manual_seed(5)) < 0.5
    half[0] = torch.arange(16)[None, :] < 8
    for sampler in ("dpmpp_2m", "ddpm"):
        out = im.sample(**text, _noise=R.make_randn(6), sample_steps=5, sampler=sampler, **start, inpaint_images=y.to(dev), inpaint_masks=half.to(dev))
        ref = restated_init_sample([sd], [16], 25, (5,), sampler, None, init=init, strengths=(0.6,), images=y, masks=half, text_embeds=emb, text_masks=mask,
                                   cond_scale=3., randn=R.make_randn(6))
        gate(out, ref, f"16^2 T=25 S=5 {sampler} init 0.6 + half mask")
        keep = half[:, None].expand_as(y)
        assert (out.cpu() - y)[keep].abs().max() <= 2. ** -22 and (out.cpu() - y)[~keep].abs().max() > 0.05
    im.check_device_status()


# ------------------------------------------------------------------------------------------------ 11. with guidance plans
@pytest.mark.parametrize("backend", BACKENDS)
def test_with_guidance_plans(backend):
    """S = 5 at T = 25: tau = 24 18 12 6 0 in execution order; strength 0.6 skips the first two.  Intervals and schedules stay indexed by the
    step of the full loop; the plan is clipped to the executed steps"""
    dev = setup(backend)
    im, sd = tiny_imagen(16, 25, dev)
    emb, mask = _captions()
    init = pixels(2, 16, 1)
    kw = dict(text_embeds=emb.to(dev), text_masks=mask.to(dev), _seed=11, sample_steps=5, init_images=init.to(dev), init_strength=0.6)
    guided = im.sample(**kw, cond_scale=3.).clone()
    unguided = im.sample(**kw, cond_scale=1.).clone()
    assert not torch.equal(guided, unguided)
    assert torch.equal(im.sample(**kw, cond_scale=3., guidance_interval=(0., 1.)), guided)
    assert torch.equal(im.sample(**kw, cond_scale=3., guidance_interval=(0.7, 1.)), unguided)          # tau 24 and 18 only: both skipped
    mixed = im.sample(**kw, cond_scale=3., guidance_interval=(0.4, 1.)).clone()                           # tau 12 of the executed ones: two runs
    assert not torch.equal(mixed, guided) and not torch.equal(mixed, unguided)
    assert torch.equal(im.sample(**kw, guidance_schedule=[[7., 7., 3., 3., 3.]]), guided)                # the skipped entries do not make it a table
    with pytest.raises(ValueError):                    # "one guided step somewhere" looks at the executed steps
        im.sample(**kw, cond_scale=3., guidance_interval=(0.7, 1.), guidance_rescale=0.5)
    ramp = [5., 4., 3., 2., 1.]
    out = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), _noise=R.make_randn(6), sample_steps=5, sampler="dpmpp_2m", init_images=init.to(dev),
                    init_strength=0.6, guidance_schedule=[ramp])
    ref = restated_init_sample([sd], [16], 25, (5,), "dpmpp_2m", None, init=init, strengths=(0.6,), scales=[ramp], text_embeds=emb, text_masks=mask,
                               randn=R.make_randn(6))
    gate(out, ref, "16^2 T=25 S=5 dpmpp_2m init 0.6 + ramp schedule")
    im.check_device_status()


# ------------------------------------------------------------------------------------------------ 12. the golden cascade (GPU)
@pytest.mark.parametrize("backend", GPU_ONLY)
@pytest.mark.parametrize("sampler", ["dpmpp_2m", "ddpm"])
def test_values_cascade(backend, sampler):
    """64 -> 256, golden weights, B = 2, T = 100, sample_steps = (10, 6), strengths (0.5, 0.5), cond_scale 3: runs of 5 and of 3 steps, the
    grouped tail of the 256^2 stage in graphs of partial length; graph == eager, and the values against the restated loop"""
    dev = setup(backend)
    im = make_imagen([64, 256], 100, dev)
    emb, mask = R.synthetic_text(2, length=48, seed=9)
    y = pixels(2, 256, 7)
    kw = dict(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., sample_steps=(10, 6), sampler=sampler, init_images=y.to(dev), init_strength=(0.5, 0.5))
    a = im.sample(**kw, _seed=11).clone()
    assert torch.equal(a, im.sample(**kw, _seed=11, _use_graph=False))
    assert a.isfinite().all() and a.std() > 0.01
    out = im.sample(**kw, _noise=R.make_randn(21))
    ref = restated_init_sample([I.load("unet0_sd.pt"), I.load("unet1_sd.pt")], [64, 256], 100, (10, 6), sampler, None, init=y, strengths=(0.5, 0.5),
                               text_embeds=emb, text_masks=mask, cond_scale=3., randn=R.make_randn(21))
    gate(out, ref, f"cascade 64->256 T=100 S=(10, 6) {sampler} init (0.5, 0.5)")
    im.check_device_status()
    sts = [v for u in im.unets for ws in u.engine()._ws.values() for v in ws.sampler_state.values()]
    assert [hasattr(v, "group_sync") for v in sts] == [False, True]
    assert sorted(e["per"] for e in sts[1].graphs.values()) == [3]
