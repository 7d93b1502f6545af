"""Imagen.sample(thresholding=, thresholding_percentile=): how x0 is bounded per stage -- the reference's dynamic threshold (with a percentile
of the call's), a static clamp to [-1, 1], or nothing.  Argument validation, the parsed StageCalls, the graph key and
forwarding (host); the one new launch mi_sampler_step_direct_fwd bit for bit against numpy; the loop against a restated loop on injected
noise (the project's gate, SURVEY.md 8(c): max|d| < 1e-4 and mean|d| < 1e-5 on [0, 1] images); the equalities of the loop (the untouched
default call, percentile, guidance plans, inpainting, init images, shards); no cooperating workgroups in a static stage."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from minimagen_amd import _lib as L
from minimagen_amd import sample_call
from minimagen_amd import sampler as S
from minimagen_amd.Imagen import Imagen
from minimagen_amd.Unet import Unet
from minimagen_amd.diffusion_model import GaussianDiffusion
from minimagen_amd.helpers import quantile_rank
from oracle import resize_restated
from oracle import restated as R
from tests import _inputs as I
from tests._backend import BACKENDS, GPU_ONLY, setup
from tests.test_sample_steps import TINY, gate, tiny_imagen

MI_ERR_INVALID = -1
MODES = ("dynamic", "static", "none")
SATURATION_CAP = {"ddpm": 0.30, "ddim": 0.30, "dpmpp_2m": 0.55}


def v_imagen(sizes, T, dev):
    """tests.test_sample_steps.make_imagen (golden weights) with U-Nets that predict v"""
    p = I.unet_params()
    unets = [Unet(**p["unet0"])] + [Unet(**p["unet1"]) for _ in sizes[1:]]
    im = Imagen(unets, text_encoder_name="t5_small", image_sizes=sizes, timesteps=T, cond_drop_prob=0.15, pred_objectives='v')
    im.unets[0].load_state_dict(I.load("unet0_sd.pt"))
    for u in im.unets[1:]:
        u.load_state_dict(I.load("unet1_sd.pt"))
    return im.to(dev)


def tiny_v_cascade(T, dev, seed=4):
    """16 -> 32, two tiny U-Nets that predict v -> (Imagen, their state dicts)"""
    torch.manual_seed(seed)
    im = Imagen([Unet(**TINY), Unet(**TINY, lowres_cond=True)], text_encoder_name="t5_small", image_sizes=[16, 32], timesteps=T, cond_drop_prob=0.15,
                pred_objectives='v')
    sds = [{k: v.clone() for k, v in u.state_dict().items()} for u in im.unets]
    return im.to(dev), sds


def restated_sample(sds, sizes, T, steps, sampler, eta, *, modes, percentiles=None, objective='v', text_embeds, text_masks, cond_scale, randn,
                    lowres_sample_noise_level=0.2):
    """tests.test_sample_steps.restated_sample with the threshold line replaced per stage: ``modes`` one of MODES per stage, ``percentiles`` the
    dynamic threshold's percentile per stage (None: 0.9); the table's columns 0 and 1 are those of ``objective``"""
    b = text_embeds.shape[0]
    steps = (steps,) * len(sds) if isinstance(steps, int) else steps
    percentiles = percentiles or (None,) * len(sds)
    lowres_sched = R.Schedule(T)
    img = None
    for sd, size, S_, mode, pct in zip(sds, sizes, steps, modes, percentiles):
        kw = dict(text_embeds=text_embeds, text_mask=text_masks, cond_scale=cond_scale)
        if "to_lowres_time_hiddens.1.weight" in sd:
            lt = lowres_sched.get_times(b, lowres_sample_noise_level)
            low = resize_restated.resize(img, scale_factors=size / img.shape[-1], pad_mode='reflect') if img.shape[-1] != size else img
            low = lowres_sched.q_sample(low, int(lt[0]), randn(low.shape))
            kw.update(lowres_cond_img=low * 2 - 1, lowres_noise_times=lt)
        tau, tab = GaussianDiffusion(timesteps=T).sampler_tables(S_, sampler, eta, objective=objective)
        shape = (b, 3, size, size)
        x, prev = randn(shape), torch.zeros(shape)
        for k in range(S_ - 1, -1, -1):
            pred = R.unet_forward_with_cond_scale(sd, x, torch.full((b,), int(tau[k]), dtype=torch.long), **kw)
            x0 = tab[k, 0] * x - tab[k, 1] * pred
            if mode == "dynamic":
                s, *_ = R.dynamic_threshold_quantile(x0.reshape(b, -1).abs(), 0.9 if pct is None else pct)
                s = s.clamp(min=1.).reshape(b, 1, 1, 1)
                x0 = x0.clamp(-s, s) / s
            elif mode == "static":
                x0 = x0.clamp(-1., 1.)
            else:
                assert mode == "none"
            z = randn(shape)
            x = ((tab[k, 2] * x0 + tab[k, 3] * x) + tab[k, 5] * prev) + tab[k, 4] * z
            prev = x0
        img = (x.clamp(-1., 1.) + 1) * 0.5
    return img


def saturated(img):
    return float(((img == 0.) | (img == 1.)).float().mean())


# ------------------------------------------------------------------------------------------------ 1. host, no backend
def _two_stage():
    return Imagen([Unet(**TINY), Unet(**TINY, lowres_cond=True)], text_encoder_name="t5_small", image_sizes=[16, 32], timesteps=25, cond_drop_prob=0.15)


def test_argument_validation():
    """bad values raise ValueError before anything is launched (no backend is loaded here: a launch would need one)"""
    im = _two_stage()
    emb, mask = R.synthetic_text(2, length=8, seed=1)
    bad = [dict(thresholding="clip"), dict(thresholding="Dynamic"), dict(thresholding=1), dict(thresholding=True),            # unknown names
           dict(thresholding=["static"]), dict(thresholding=["static"] * 3), dict(thresholding=("none", "clip")),                # lengths, an entry
           dict(thresholding=[None, 0.5]),
           dict(thresholding_percentile=1.5), dict(thresholding_percentile=-0.1), dict(thresholding_percentile=True),
           dict(thresholding_percentile=float("nan")), dict(thresholding_percentile="0.5"),
           dict(thresholding_percentile=[0.5]), dict(thresholding_percentile=[0.5] * 3), dict(thresholding_percentile=[0.5, True]),
           dict(thresholding_percentile=[None, 2.]),
           dict(thresholding="static", thresholding_percentile=0.5), dict(thresholding="none", thresholding_percentile=0.5),   # a percentile without the dynamic mode
           dict(thresholding=["dynamic", "static"], thresholding_percentile=0.5),
           dict(thresholding=["static", None], thresholding_percentile=[0.5, None]),
           dict(thresholding=["dynamic", "none"], thresholding_percentile=[None, 0.5]),
           dict(thresholding=["static", "dynamic"], thresholding_percentile=[None, 1.5], stop_at_stage=1)]                      # (every entry's VALUE is validated)
    for kw in bad:
        with pytest.raises(ValueError):
            im.sample(text_embeds=emb, text_masks=mask, **kw)
    with pytest.raises(TypeError):
        im.sample(emb, None, None, 1., None, False, None, "static")          # keyword-only
    assert "thresholding" in Imagen.sample.__doc__ and "thresholding_percentile" in Imagen.sample.__doc__


def _stages(im, **kw):
    emb, mask = R.synthetic_text(2, length=8, seed=1)
    names = sample_call.parse.__code__.co_varnames[1:sample_call.parse.__code__.co_kwonlyargcount + 1]
    args = {k: None for k in names}
    args.update(text_embeds=emb, text_masks=mask, cond_scale=1., return_pil_images=False, _seed=1, _sample_offset=0, _use_graph=True, _async=False)
    args.update(kw)
    return sample_call.parse(im, **args).stages


def test_parsed_stage_calls():
    im = _two_stage()
    fields = lambda **kw: [(s.stage, s.threshold, s.percentile) for s in _stages(im, **kw)]
    assert fields(thresholding="dynamic") == fields(thresholding=None) == [(0, "dynamic", None), (1, "dynamic", None)]
    assert fields(thresholding="static") == [(0, "static", None), (1, "static", None)]
    assert fields(thresholding=("none", None)) == [(0, "none", None), (1, "dynamic", None)]
    assert fields(thresholding=[None, "static"], thresholding_percentile=[0.5, None]) == [(0, "dynamic", 0.5), (1, "static", None)]
    assert fields(thresholding="dynamic", thresholding_percentile=1) == [(0, "dynamic", 1.), (1, "dynamic", 1.)]
    assert fields(thresholding="dynamic", thresholding_percentile=0) == [(0, "dynamic", 0.), (1, "dynamic", 0.)]
    # a stage the call does not run is ignored: its percentile may sit on a static entry
    assert fields(thresholding=["dynamic", "static"], thresholding_percentile=0.5, stop_at_stage=1) == [(0, "dynamic", 0.5)]
    assert fields(thresholding=["static", "dynamic"], thresholding_percentile=[0.25, 0.5], start_at_stage=1, start_image=torch.rand(2, 3, 16, 16)) == [(1, "dynamic", 0.5)]
    # the default StageCall stays the reference's loop, and the default parse is that StageCall
    d = S.StageCall(0, 25)
    assert (d.threshold, d.percentile) == ("dynamic", None) and d.state_key(25) == 25
    plain = _stages(im, thresholding="dynamic")
    assert plain == _stages(im, thresholding="dynamic", thresholding_percentile=None) and plain[0].state_key(25) == 25
    assert _stages(im, thresholding="static")[0].state_key(25) == 25           # no table depends on the mode


def test_graph_key():
    """a default call's key is the tuple it always was, element for element; a mode adds ("thr", mode) behind everything else"""
    rank = quantile_rank(768, 0.9)
    d = S.StageCall(0, 25)
    assert S.graph_key(d, 3., True, rank, 0, True, False, False, 0., False) == (3.0, True, rank[0], rank[1], rank[2], 0, 0, 25, True, False)
    solver = S.StageCall(1, 10, (10, "ddim", 0.5))
    full = (2.0, False, *rank, 4, 1, 10, False, True, (10, "ddim", 0.5), "inpaint", ("rescale", 0.7), "sched", ("len", 3))
    assert S.graph_key(solver, 2., False, rank, 4, False, True, True, 0.7, True, 3) == full
    for mode in ("static", "none"):
        m = S.StageCall(1, 10, (10, "ddim", 0.5), threshold=mode)
        assert S.graph_key(m, 2., False, rank, 4, False, True, True, 0.7, True, 3) == full + (("thr", mode),)
        assert S.graph_key(S.StageCall(0, 25, threshold=mode), 3., True, rank, 0, True, False, False, 0., False)[-1] == ("thr", mode)
    # a percentile of the call's is in the rank, nowhere else
    p = S.StageCall(0, 25, percentile=0.5)
    assert S.graph_key(p, 3., True, rank, 0, True, False, False, 0., False) == S.graph_key(d, 3., True, rank, 0, True, False, False, 0., False)
    assert quantile_rank(768, 0.5) != rank


def test_forwarding_entry_points_pass_the_keywords(tmp_path):
    """generate.sample_and_save(sample_args=) and distributed.sample_distributed(**kwargs) hand the two keywords to Imagen.sample unchanged (a
    recording stand-in for the model: no backend needed) and say so in their docstrings"""
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

    knobs = dict(thresholding=["dynamic", "static"], thresholding_percentile=[0.5, None])
    generate.sample_and_save(["a", "b"], minimagen=Recorder(), sample_args=dict(cond_scale=3., **knobs), save_directory=str(tmp_path / "out"))
    assert all(seen[-1][k] is v for k, v in knobs.items()) and seen[-1]["cond_scale"] == 3.
    out = distributed.sample_distributed(Recorder(), text_embeds=torch.zeros(3, 4, 16), thresholding="none")
    assert out.shape[0] == 3 and seen[-1]["thresholding"] == "none" and "thresholding_percentile" not in seen[-1] and seen[-1]["_sample_offset"] == 0
    distributed.sample_distributed(Recorder(), text_embeds=torch.zeros(3, 4, 16), thresholding_percentile=0.75)
    assert seen[-1]["thresholding_percentile"] == 0.75
    for fn in (generate.sample_and_save, distributed.sample_distributed):
        assert "thresholding" in fn.__doc__ and "thresholding_percentile" in fn.__doc__


# ------------------------------------------------------------------------------------------------ 2. the launch, bit for bit
def _bits(a):
    return (a.cpu().numpy() if torch.is_tensor(a) else a).view(np.uint32)


def _same(got, want):
    """all bits, but for NaN elements: those must be NaN on both sides"""
    got, want = (a.cpu().numpy() if torch.is_tensor(a) else a for a in (got, want))
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


def _np_guided_x0(pred2, xt, row, two, scale):
    """the stated order, one rounding per operation: pred = null + (cond - null) * scale; x0 = c0 x_t - c1 pred"""
    f = np.float32
    B = xt.shape[0]
    pred = pred2[:B]
    if two:
        pred = (pred2[B:] + ((pred2[:B] - pred2[B:]).astype(f) * f(scale)).astype(f)).astype(f)
    return ((f(row[0]) * xt).astype(f) - (f(row[1]) * pred).astype(f)).astype(f)


def _np_direct_step(x0, xt, prev, z, row, clip, known=None):
    """clip (1: clamp to [-1, 1], NaN stays NaN; 0: nothing); mean = c2 x0 + c3 x; mean += c5 prev (history); x' = mean + c4 z; then the masked
    replace x' = m ? c6 y + c7 z' : x' (at row 0, ``known`` = (m, y, None): y itself).  -> (x', the x0 the history keeps)"""
    f = np.float32
    if clip:
        x0 = np.where(np.isnan(x0), x0, np.minimum(np.maximum(x0, f(-1)), f(1))).astype(f)
    mean = ((f(row[2]) * x0).astype(f) + (f(row[3]) * xt).astype(f)).astype(f)
    if prev is not None:
        mean = (mean + (f(row[5]) * prev).astype(f)).astype(f)
    x = (mean + (f(row[4]) * z).astype(f)).astype(f)
    if known is not None:
        m, y, zk = known
        x = np.where(m, y if zk is None else ((f(row[6]) * y).astype(f) + (f(row[7]) * zk).astype(f)).astype(f), x).astype(f)
    return x, x0


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("n", [3 * 16 * 16, 3 * 5 * 5, 8, 3 * 76 * 76])
def test_direct_tail_bit_exact(backend, n):
    """mi_sampler_step_direct_fwd on injected step and known-region noise against numpy in the stated operation order, all bits of x and of
    x0_prev: two in {0, 1} x history x inpainting x clip, at a middle row (history coefficient != 0), behind a t_off, and at row 0 (the last
    blend: no draw).  16-byte accesses (768, 8, 17328: several workgroups per image and a partial last one), element by element with a ragged
    quad and mask quads that straddle channels (75).  x0 has elements below -1, inside and above 1, and one NaN"""
    dev = setup(backend)
    lib, st = L.lib(), L.current_stream()
    B, T, S_ = 2, 100, 10
    hw = n // 3 if n % 3 == 0 else 4
    _, tab = GaussianDiffusion(timesteps=T).sampler_tables(S_, "dpmpp_2m", known=True)
    coef = tab.to(dev).contiguous()
    g = torch.Generator().manual_seed(n)
    pred2, xt = torch.randn(2 * B, n, generator=g) * 1.5, torch.randn(B, n, generator=g)
    pred2[0, 2] = float("nan")
    noise, known_noise, prev0 = torch.randn(S_, B, n, generator=g), torch.randn(S_, B, n, generator=g), torch.randn(B, n, generator=g)
    y = torch.rand(B, n, generator=g) * 2 - 1
    m8 = (torch.rand(B, hw, generator=g) < 0.5).to(torch.uint8)
    m8[0, :2] = torch.tensor([1, 0], dtype=torch.uint8)
    mfull = m8.bool().repeat(1, n // hw).numpy()
    noised, knd, yd, m8d = (t.to(dev).contiguous() for t in (noise, known_noise, y, m8))
    ip = L.MiInpaintParams(yd.data_ptr(), m8d.data_ptr(), hw, 0, knd.data_ptr())
    rows_pred = pred2
    for k, off in ((5, 0), (3, 2), (0, 0)):
        row = tab[k].numpy()
        tstate = torch.tensor([k + off], dtype=torch.int32, device=dev)
        # three elements of image 1 get a prediction (the same in both halves: the guidance combine returns it) that puts x0 near -2, 0.3 and 2
        pred2 = rows_pred.clone()
        for j, target in enumerate((-2., 0.3, 2.)):
            pred2[1, j] = pred2[B + 1, j] = (tab[k, 0] * xt[1, j] - target) / tab[k, 1]
        pred2d = pred2.to(dev).contiguous()
        for two in (0, 1):
            x0 = _np_guided_x0(pred2.numpy(), xt.numpy(), row, two, 3.0)
            assert abs(x0[1, 0] + 2) < 0.1 and abs(x0[1, 1] - 0.3) < 0.1 and abs(x0[1, 2] - 2) < 0.1
            fin = x0[~np.isnan(x0)]
            assert (fin < -1).any() and (np.abs(fin) <= 1).any() and (fin > 1).any() and np.isnan(x0).sum() == 1
            for hist in (False, True):
                for inpaint in (False, True):
                    for clip in (1, 0):
                        buf = torch.full((B * n + 8,), 7., device=dev)
                        buf[:B * n] = xt.reshape(-1).to(dev)
                        x, pv = buf[:B * n], prev0.clone().to(dev)
                        cp = L.MiCfgX0Params(B, n, pred2d.data_ptr(), two, 3.0, x.data_ptr(), coef.data_ptr(), tstate.data_ptr(), 0, 0, 0, off)
                        pp = L.MiPosteriorParams(B, n, S_, 0, 0, x.data_ptr(), coef.data_ptr(), tstate.data_ptr(), noised.data_ptr(), 0, 0, 0, 0, off)
                        ext = L.MiSamplerExtParams(0, pv.data_ptr() if hist else 0)
                        L.check(lib.mi_sampler_step_direct_fwd(C.byref(cp), C.byref(pp), C.byref(ext), C.byref(ip) if inpaint else None, clip, st),
                                "mi_sampler_step_direct_fwd")
                        if backend == "gpu":
                            torch.cuda.synchronize()
                        known = (mfull, y.numpy(), known_noise[S_ - k].numpy() if k > 0 else None) if inpaint else None
                        want_x, want_prev = _np_direct_step(x0, xt.numpy(), prev0.numpy() if hist else None, noise[S_ - 1 - k].numpy(), row, clip, known)
                        what = (k, off, two, hist, inpaint, clip)
                        assert _same(x.reshape(B, n), want_x), what
                        assert (buf[B * n:] == 7.).all(), what                         # nothing behind the rows is written
                        assert _same(pv, want_prev) if hist else torch.equal(pv.cpu(), prev0), what
                        if clip == 1 and not inpaint:
                            assert np.isnan(want_x).sum() == 1                          # the NaN stays NaN through the clamp
    # e == NULL is e without x0_prev
    xa, xb = xt.clone().to(dev), xt.clone().to(dev)
    tstate = torch.tensor([5], dtype=torch.int32, device=dev)
    for x, e in ((xa, None), (xb, C.byref(L.MiSamplerExtParams(0, 0)))):
        cp = L.MiCfgX0Params(B, n, pred2d.data_ptr(), 1, 3.0, x.data_ptr(), coef.data_ptr(), tstate.data_ptr(), 0, 0, 0, 0)
        pp = L.MiPosteriorParams(B, n, S_, 0, 0, x.data_ptr(), coef.data_ptr(), tstate.data_ptr(), noised.data_ptr(), 0, 0, 0, 0, 0)
        L.check(lib.mi_sampler_step_direct_fwd(C.byref(cp), C.byref(pp), e, None, 1, st))
    assert torch.equal(xa.view(torch.int32), xb.view(torch.int32))
    assert lib.mi_abi_version() == 12 and lib.mi_struct_size(30) == -1 and lib.mi_struct_size(35) == -1


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("n", [3 * 16 * 16, 3 * 5 * 5, 8, 3 * 76 * 76])
def test_direct_tail_philox_equals_the_dynamic_tails_at_scale_one(backend, n):
    """on-device noise: where every |x0| <= 1 the dynamic scale is exactly 1 (asserted on the tail's own s_out), so the static clamp, no clamp, the
    one-workgroup tail (where the image fits it) and the separate kernels must give the same bits of x and of x0_prev from the same seed"""
    dev = setup(backend)
    lib, st = L.lib(), L.current_stream()
    B, T, S_, k = 2, 100, 10, 5
    _, tab = GaussianDiffusion(timesteps=T).sampler_tables(S_, "dpmpp_2m")
    coef = tab.to(dev).contiguous()
    g = torch.Generator().manual_seed(n + 1)
    pred2, xt, prev0 = torch.randn(2 * B, n, generator=g), torch.randn(B, n, generator=g), torch.randn(B, n, generator=g)
    shrink = 0.5 / float(np.abs(_np_guided_x0(pred2.numpy(), xt.numpy(), tab[k].numpy(), 1, 3.0)).max())          # (x0 is linear in its inputs)
    pred2, xt = pred2 * shrink, xt * shrink
    x0 = _np_guided_x0(pred2.numpy(), xt.numpy(), tab[k].numpy(), 1, 3.0)
    assert 0.4 < np.abs(x0).max() <= 1
    pred2d = pred2.to(dev)
    tstate = torch.tensor([k], dtype=torch.int32, device=dev)
    k_lo, k_hi, w = quantile_rank(n, 0.9)
    seeded = lambda x: L.MiPosteriorParams(B, n, S_, 0, 0, x.data_ptr(), coef.data_ptr(), tstate.data_ptr(), 0, 77, 5, 3 << 20, 0, 0)
    results = {}
    for clip in (1, 0):
        x, pv = xt.clone().to(dev), prev0.clone().to(dev)
        cp = L.MiCfgX0Params(B, n, pred2d.data_ptr(), 1, 3.0, x.data_ptr(), coef.data_ptr(), tstate.data_ptr(), 0, 0, 0, 0)
        L.check(lib.mi_sampler_step_direct_fwd(C.byref(cp), C.byref(seeded(x)), C.byref(L.MiSamplerExtParams(0, pv.data_ptr())), None, clip, st))
        results[f"clip {clip}"] = (x, pv)
    if n <= 16384:
        x, pv, s_q = xt.clone().to(dev), prev0.clone().to(dev), torch.full((B,), 9., device=dev)
        cp = L.MiCfgX0Params(B, n, pred2d.data_ptr(), 1, 3.0, x.data_ptr(), coef.data_ptr(), tstate.data_ptr(), 0, 0, 0, 0)
        qp = L.MiQuantileParams(B, n, 0, k_lo, k_hi, w, 0, s_q.data_ptr(), 0, 0, 0)
        L.check(lib.mi_sampler_step_small_ext_fwd(C.byref(cp), C.byref(qp), C.byref(seeded(x)), C.byref(L.MiSamplerExtParams(0, pv.data_ptr())), st))
        assert (s_q <= 1).all() and (s_q > 0).all()
        results["small"] = (x, pv)
    x, pv, s_q, x0d = xt.clone().to(dev), prev0.clone().to(dev), torch.full((B,), 9., device=dev), torch.zeros(B, n, device=dev)
    hist = torch.zeros(3 * B * 2 * 2048, dtype=torch.int32, device=dev)
    cp = L.MiCfgX0Params(B, n, pred2d.data_ptr(), 1, 3.0, x.data_ptr(), coef.data_ptr(), tstate.data_ptr(), 0, x0d.data_ptr(), 0, 0)
    L.check(lib.mi_cfg_x0_fwd(C.byref(cp), st))
    L.check(lib.mi_quantile_fwd(C.byref(L.MiQuantileParams(B, n, x0d.data_ptr(), k_lo, k_hi, w, hist.data_ptr(), s_q.data_ptr(), None)), st))
    pr = seeded(x)
    pr.x0, pr.s_q = x0d.data_ptr(), s_q.data_ptr()
    L.check(lib.mi_posterior_ext_fwd(C.byref(pr), C.byref(L.MiSamplerExtParams(0, pv.data_ptr())), st))
    assert (s_q <= 1).all() and (s_q > 0).all()                       # the condition of the equality, not luck
    assert np.array_equal(_bits(x0d), _bits(x0))
    results["separate"] = (x, pv)
    ref_x, ref_pv = results["separate"]
    assert not torch.equal(ref_x.cpu(), xt)
    for name, (x, pv) in results.items():
        assert torch.equal(x, ref_x) and torch.equal(pv, ref_pv), name


@pytest.mark.parametrize("backend", BACKENDS)
def test_direct_tail_bad_arguments(backend):
    dev = setup(backend)
    lib, st = L.lib(), L.current_stream()
    B, n = 2, 48
    coef = GaussianDiffusion(timesteps=100).sampler_tables(10, "ddpm", known=True)[1].to(dev).contiguous()
    pred2, x, other = torch.zeros(2 * B, n, device=dev), torch.zeros(B, n, device=dev), torch.zeros(B, n, device=dev)
    noise = torch.zeros(10, B, n, device=dev)
    tstate, tstate2 = torch.tensor([5], dtype=torch.int32, device=dev), torch.tensor([5], dtype=torch.int32, device=dev)
    m8 = torch.zeros(B, 16, dtype=torch.uint8, device=dev)

    def blocks():
        return (L.MiCfgX0Params(B, n, pred2.data_ptr(), 1, 3.0, x.data_ptr(), coef.data_ptr(), tstate.data_ptr(), 0, 0, 0, 0),
                L.MiPosteriorParams(B, n, 10, 0, 0, x.data_ptr(), coef.data_ptr(), tstate.data_ptr(), noise.data_ptr(), 0, 0, 0, 0, 0))

    call = lambda cp, pp, ip=None, clip=1: lib.mi_sampler_step_direct_fwd(C.byref(cp), C.byref(pp), None, None if ip is None else C.byref(ip), clip, st)
    assert call(*blocks()) == 0 and call(*blocks(), clip=0) == 0
    for clip in (2, -1, 3):
        assert call(*blocks(), clip=clip) == MI_ERR_INVALID and b"clip" in lib.mi_last_error()

    def broken(which, field, value):
        cp, pp = blocks()
        setattr((cp, pp)[which], field, value)
        return call(cp, pp)

    for which, field, value in ((1, "B", B + 1), (1, "n", n - 4), (0, "B", 0), (0, "n", 0), (1, "x", other.data_ptr()), (0, "x_t", 0), (0, "coef", 0),
                                (1, "coef", coef.data_ptr() + 32), (1, "t_state", tstate2.data_ptr()), (1, "t_off", 1), (0, "t_state", 0)):
        assert broken(which, field, value) == MI_ERR_INVALID, (which, field)
    for ip in (L.MiInpaintParams(0, m8.data_ptr(), 16, 0, 0), L.MiInpaintParams(other.data_ptr(), 0, 16, 0, 0), L.MiInpaintParams(other.data_ptr(), m8.data_ptr(), 0, 0, 0),
               L.MiInpaintParams(other.data_ptr(), m8.data_ptr(), 7, 0, 0)):
        assert call(*blocks(), ip=ip) == MI_ERR_INVALID and b"inpaint" in lib.mi_last_error()
    assert call(*blocks(), ip=L.MiInpaintParams(other.data_ptr(), m8.data_ptr(), 16, 0, 0)) == 0


# ------------------------------------------------------------------------------------------------ 3. values against the restated loop
def _captions(B=2, length=16, seed=7):
    return R.synthetic_text(B, length=length, seed=seed)


@functools.lru_cache(maxsize=None)
def _golden_reference(sampler, mode):
    emb, mask = _captions()
    return restated_sample([I.load("unet0_sd.pt")], [32], 100, 6, sampler, None, modes=(mode,), text_embeds=emb, text_masks=mask, cond_scale=3.,
                           randn=R.make_randn(3))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("mode", ["static", "none"])
@pytest.mark.parametrize("sampler", ["ddpm", "ddim", "dpmpp_2m"])
def test_values_one_stage(backend, sampler, mode):
    """32^2, golden base weights predicting v, B = 2, T = 100, S = 6, cond_scale 3.  The final clamp can hide errors: at most SATURATION_CAP of the
    reference's pixels sit at exactly 0 or 1; and the three modes' references differ by more than 100 x the gate, so a mode that fell back to
    another one fails"""
    dev = setup(backend)
    im = v_imagen([32], 100, dev)
    emb, mask = _captions()
    out = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., _noise=R.make_randn(3), sample_steps=6, sampler=sampler, thresholding=mode)
    im.check_device_status()
    refs = {m: _golden_reference(sampler, m) for m in MODES}
    share = saturated(refs[mode])
    print(f"{sampler} {mode}: saturated share of the reference {share:.3f}")
    assert share <= SATURATION_CAP[sampler], share
    for a in MODES:
        for b in MODES:
            if a < b:
                d = (refs[a] - refs[b]).abs().max()
                print(f"{sampler}: max|{a} - {b}| = {d:.3f}")
                assert d > 100 * 1e-4, (a, b, d)
    gate(out, refs[mode], f"32^2 v T=100 S=6 {sampler} thresholding={mode}")
    assert im._status_stages == [] and not im._status_pending


# ------------------------------------------------------------------------------------------------ 4. per-stage routing: a tiny 16 -> 32 cascade
@functools.lru_cache(maxsize=None)
def _cascade_reference(modes, percentiles):
    _, sds = tiny_v_cascade(25, torch.device("cpu"))
    emb, mask = _captions()
    return restated_sample(sds, [16, 32], 25, (4, 3), "ddpm", None, modes=modes, percentiles=percentiles, text_embeds=emb, text_masks=mask, cond_scale=3.,
                           randn=R.make_randn(8))


@pytest.mark.parametrize("backend", BACKENDS)
def test_values_cascade_tiny(backend):
    """16 -> 32 tiny (v), B = 2, T = 25, S = (4, 3), 'ddpm': the base stage dynamic at percentile 0.5, the super-resolution stage static behind
    the low-resolution conditioning path -- and both choices really change the image"""
    dev = setup(backend)
    im, _ = tiny_v_cascade(25, dev)
    emb, mask = _captions()
    out = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., _noise=R.make_randn(8), sample_steps=(4, 3), sampler="ddpm",
                    thresholding=["dynamic", "static"], thresholding_percentile=[0.5, None])
    im.check_device_status()
    ref = _cascade_reference(("dynamic", "static"), (0.5, None))
    share = saturated(ref)
    print(f"tiny cascade: saturated share of the reference {share:.3f}")
    assert share <= SATURATION_CAP["ddpm"], share
    for other in ((("dynamic", "static"), (None, None)), (("dynamic", "dynamic"), (0.5, None))):
        assert (ref - _cascade_reference(*other)).abs().max() > 100 * 1e-4, other
    gate(out, ref, "16->32 tiny v T=25 S=(4, 3) ddpm thresholding=[dynamic @ 0.5, static]")
    sts = [v for u in im.unets for ws in u.engine()._ws.values() for v in ws.sampler_state.values()]
    assert len(sts) == 2 and not any(hasattr(v, "group_sync") for v in sts)


# ------------------------------------------------------------------------------------------------ 5. equalities, bit for bit
def _tiny(S_img, T, dev, **kw):
    """tests.test_sample_steps.tiny_imagen with constructor keywords (same seed: same weights)"""
    torch.manual_seed(4)
    return Imagen([Unet(**TINY)], text_encoder_name="t5_small", image_sizes=[S_img], timesteps=T, cond_drop_prob=0.15, **kw).to(dev)


@pytest.mark.parametrize("backend", BACKENDS)
def test_default_call_is_untouched(backend):
    """thresholding='dynamic' alone IS the plain call: same bits, the same one cached graph, the same key as ever"""
    dev = setup(backend)
    gpu = backend == "gpu"
    T = 25 if gpu else 21                                  # (the emulator takes ~1 s per step)
    im, _ = tiny_imagen(16, T, dev)
    emb, mask = _captions()
    kw = dict(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., _seed=11)
    a = im.sample(**kw).clone()
    sts = next(iter(im.unets[0].engine()._ws.values())).sampler_state
    keys = list(sts[T].graphs)
    assert list(sts) == [T] and len(keys) == 1
    assert keys[0] == (3.0, True, *quantile_rank(768, 0.9), 0, 0, T, True, False)
    assert torch.equal(im.sample(**kw, thresholding="dynamic"), a)
    if gpu:
        assert torch.equal(im.sample(**kw, thresholding=["dynamic"], thresholding_percentile=[None]), a)
    assert list(sts) == [T] and list(sts[T].graphs) == keys
    b = im.sample(**kw, thresholding="static").clone()
    assert list(sts) == [T] and list(sts[T].graphs) == keys + [keys[0] + (("thr", "static"),)]
    assert not torch.equal(a, b)
    if gpu:
        assert torch.equal(im.sample(**kw), a) and torch.equal(im.sample(**kw, thresholding="static"), b)
        assert torch.equal(b, im.sample(**kw, thresholding="static", _use_graph=False))
    im.check_device_status()


@pytest.mark.parametrize("backend", BACKENDS)
def test_percentile_of_the_call(backend):
    dev = setup(backend)
    emb, mask = _captions()
    kw = dict(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., _seed=11, sample_steps=5)
    im, built = _tiny(16, 25, dev), _tiny(16, 25, dev, dynamic_thresholding_percentile=0.5)
    plain = im.sample(**kw).clone()
    a = im.sample(**kw, thresholding_percentile=0.5).clone()
    assert torch.equal(a, built.sample(**kw)) and not torch.equal(a, plain)
    assert torch.equal(im.sample(**kw, thresholding_percentile=0.9), plain) and im.dynamic_thresholding_percentile == 0.9
    im.check_device_status()


@pytest.mark.parametrize("backend", BACKENDS)
def test_static_with_guidance_plans_inpainting_init_and_shards(backend):
    dev = setup(backend)
    im, _ = tiny_imagen(16, 25, dev)
    emb, mask = _captions(4)
    emb, mask = emb.to(dev), mask.to(dev)
    two = dict(text_embeds=emb[:2].contiguous(), text_masks=mask[:2].contiguous(), cond_scale=3., _seed=11, sample_steps=5, sampler="dpmpp_2m", thresholding="static")
    plain = im.sample(**two).clone()
    # guidance plans: (0, 1) is the call itself; an interval that splits the stage into runs (tau = 24 18 12 6 0) replays what it runs eagerly
    assert torch.equal(im.sample(**two, guidance_interval=(0., 1.)), plain)
    split = im.sample(**two, guidance_interval=(0.4, 1.)).clone()
    assert not torch.equal(split, plain) and torch.equal(split, im.sample(**two, guidance_interval=(0.4, 1.), _use_graph=False))
    # shards
    whole = im.sample(**{**two, "text_embeds": emb, "text_masks": mask})
    assert torch.equal(whole[:2], plain)
    part = im.sample(**{**two, "text_embeds": emb[2:].contiguous(), "text_masks": mask[2:].contiguous()}, _sample_offset=2)
    assert torch.equal(part, whole[2:]) and not torch.equal(part, plain)
    assert im._status_stages == [] and not im._status_pending
    # inpainting: the known pixels are the resized known image's bits (no normalisation: no rounding between the image and the output)
    im.auto_normalize_img = False
    g = torch.Generator().manual_seed(5)
    y = (torch.rand(2, 3, 24, 24, generator=g) * 1.2 - 0.1).to(dev)
    half = torch.rand(2, 16, 16, generator=g) < 0.5
    out = im.sample(**two, inpaint_images=y, inpaint_masks=half.to(dev)).cpu()
    if backend == "gpu":
        torch.cuda.synchronize()
    ws = next(iter(im.unets[0].engine()._ws.values()))
    at_size = S.cubic_resize(ws, y.contiguous(), 16, L.current_stream())
    if backend == "gpu":
        torch.cuda.synchronize()
    keep = half[:, None].expand(2, 3, 16, 16)
    assert torch.equal(out[keep], at_size.cpu().clamp(0., 1.)[keep]) and (out[~keep] - at_size.cpu().clamp(0., 1.)[~keep]).abs().max() > 0.05
    im.check_device_status()


@pytest.mark.parametrize("backend", BACKENDS)
def test_static_full_strength_init_at_T20_is_the_plain_static_call(backend):
    """as tests.test_init_image.test_full_strength_at_T20_is_the_plain_call: at T = 20 the level of x_T is (0, 1), so init_strength = 1 starts
    from the x_T draw itself; column 0 of the first row is inf there, so the images are compared as bit patterns"""
    dev = setup(backend)
    im, _ = tiny_imagen(16, 20, dev)
    emb, mask = _captions()
    kw = dict(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., _seed=11, thresholding="static")
    y = torch.rand(2, 3, 24, 24, generator=torch.Generator().manual_seed(3)).to(dev)
    for solver in ((dict(), dict(sampler="ddim", sample_steps=7)) if backend == "gpu" else (dict(sampler="ddim", sample_steps=7),)):
        a = im.sample(**kw, **solver).clone()
        b = im.sample(**kw, **solver, init_images=y, init_strength=1.)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), solver
    ws = next(iter(im.unets[0].engine()._ws.values()))
    assert all(len(v.graphs) == 1 and list(v.graphs)[0][-1] == ("thr", "static") for v in ws.sampler_state.values())
    im.check_device_status()


# ------------------------------------------------------------------------------------------------ 6. no cooperating workgroups
@pytest.mark.parametrize("backend", BACKENDS)
def test_static_stage_above_the_small_tail_has_no_group_state(backend):
    """an image too large for the one-workgroup tail: the dynamic call takes the grouped tail there (tests.test_sample_steps), a static one the
    direct tail -- no sync buffer, no status word to poll"""
    dev = setup(backend)
    size = 96 if backend == "gpu" else 76
    assert 3 * size * size > 16384
    im, _ = tiny_imagen(size, 25, dev)
    emb, mask = R.synthetic_text(2, length=10, seed=3)
    out = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=2., _seed=11, sample_steps=3, thresholding="static")
    assert im._status_stages == [] and not im._status_pending
    im.check_device_status()
    assert out.isfinite().all() and out.std() > 0.01
    sts = list(next(iter(im.unets[0].engine()._ws.values())).sampler_state.values())
    assert len(sts) == 1 and getattr(sts[0], "group_sync", None) is None and sts[0].group_err_host is None


# ------------------------------------------------------------------------------------------------ 7. the golden cascade (GPU)
@pytest.mark.parametrize("backend", GPU_ONLY)
def test_values_cascade(backend):
    """64 -> 256, golden weights predicting v, B = 2, T = 100, sample_steps = (6, 4), 'ddpm', cond_scale 3, static: the 256^2 direct tail behind
    the folded super-resolution U-Net"""
    dev = setup(backend)
    im = v_imagen([64, 256], 100, dev)
    emb, mask = R.synthetic_text(2, length=48, seed=9)
    out = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., _noise=R.make_randn(21), sample_steps=(6, 4), sampler="ddpm",
                    thresholding="static")
    ref = restated_sample([I.load("unet0_sd.pt"), I.load("unet1_sd.pt")], [64, 256], 100, (6, 4), "ddpm", None, modes=("static", "static"), text_embeds=emb,
                          text_masks=mask, cond_scale=3., randn=R.make_randn(21))
    share = saturated(ref)
    print(f"cascade 64->256 static: saturated share of the reference {share:.3f}")
    assert share <= SATURATION_CAP["ddpm"], share
    gate(out, ref, "cascade 64->256 v T=100 S=(6, 4) ddpm thresholding=static")
    im.check_device_status()
    assert im._status_stages == [] and not im._status_pending
    sts = [v for u in im.unets for ws in u.engine()._ws.values() for v in ws.sampler_state.values()]
    assert len(sts) == 2 and not any(hasattr(v, "group_sync") for v in sts)
