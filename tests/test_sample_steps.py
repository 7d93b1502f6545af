"""Imagen.sample(sample_steps=, sampler=, sampler_eta=): sampling in fewer steps than the schedule has -- strided DDPM, DDIM and
DPM-Solver++ 2M over a subsequence of the trained timesteps.  The tables (host, fp64 identities), the kernels behind them (the history
term of the three sampler tails, the mapped step kernels), the values against a restated loop on injected noise (the project's gate,
SURVEY.md 8(c): max|d| < 1e-4 and mean|d| < 1e-5 on [0, 1] images) and the invariants of the sampling loop."""
import ctypes as C

import numpy as np
import pytest
import torch

from minimagen_amd import _lib as L
from minimagen_amd.Imagen import Imagen
from minimagen_amd.Unet import Unet
from minimagen_amd.diffusion_model import GaussianDiffusion
from minimagen_amd.helpers import quantile_rank
from oracle import resize_restated
from oracle import restated as R
from tests import _inputs as I
from tests._backend import BACKENDS, GPU_ONLY, setup

SOLVERS = [("ddpm", None), ("ddim", None), ("ddim", 0.5), ("dpmpp_2m", None)]
TINY = dict(dim=8, dim_mults=(1, 2), num_resnet_blocks=1, layer_attns=False, layer_cross_attns=False, memory_efficient=True)


def make_imagen(sizes, T, dev, cond_drop_prob=0.15):
    p = I.unet_params()
    unets = [Unet(**p["unet0"])] + [Unet(**p["unet1"]) for _ in sizes[1:]]
    im = Imagen(unets, text_encoder_name="t5_small", image_sizes=sizes, timesteps=T, cond_drop_prob=cond_drop_prob)
    im.unets[0].load_state_dict(I.load("unet0_sd.pt"))
    for u in im.unets[1:]:
        u.load_state_dict(I.load("unet1_sd.pt"))
    return im.to(dev)


def tiny_imagen(S, T, dev, seed=4):
    torch.manual_seed(seed)
    im = Imagen([Unet(**TINY)], text_encoder_name="t5_small", image_sizes=[S], timesteps=T, cond_drop_prob=0.15)
    sd = {k: v.clone() for k, v in im.unets[0].state_dict().items()}
    return im.to(dev), sd


def restated_sample(sds, sizes, T, steps, sampler, eta, *, text_embeds, text_masks, cond_scale, randn, lowres_sample_noise_level=0.2):
    """oracle.restated.sample with the S-step loop restated on the host: the step at trained timestep tau_k from row k of the fp32 table, in
    fp32 torch ops in the kernels' operation order; draw order x_T, then one draw per step (every solver); the cascade's plumbing as R.sample"""
    b = text_embeds.shape[0]
    steps = (steps,) * len(sds) if isinstance(steps, int) else steps
    lowres_sched = R.Schedule(T)
    img = None
    for sd, size, S in zip(sds, sizes, steps):
        kw = dict(text_embeds=text_embeds, text_mask=text_masks, cond_scale=cond_scale)
        if "to_lowres_time_hiddens.1.weight" in sd:
            lt = lowres_sched.get_times(b, lowres_sample_noise_level)
            low = resize_restated.resize(img, scale_factors=size / img.shape[-1], pad_mode='reflect') if img.shape[-1] != size else img
            low = lowres_sched.q_sample(low, int(lt[0]), randn(low.shape))
            kw.update(lowres_cond_img=low * 2 - 1, lowres_noise_times=lt)
        tau, tab = GaussianDiffusion(timesteps=T).sampler_tables(S, sampler, eta)
        shape = (b, 3, size, size)
        x, prev = randn(shape), torch.zeros(shape)
        for k in range(S - 1, -1, -1):
            pred = R.unet_forward_with_cond_scale(sd, x, torch.full((b,), int(tau[k]), dtype=torch.long), **kw)
            x0 = tab[k, 0] * x - tab[k, 1] * pred
            s, *_ = R.dynamic_threshold_quantile(x0.reshape(b, -1).abs(), 0.9)
            s = s.clamp(min=1.).reshape(b, 1, 1, 1)
            x0 = x0.clamp(-s, s) / s
            z = randn(shape)
            x = ((tab[k, 2] * x0 + tab[k, 3] * x) + tab[k, 5] * prev) + tab[k, 4] * z
            prev = x0
        img = (x.clamp(-1., 1.) + 1) * 0.5
    return img


def gate(out, ref, what):
    d = (out.cpu() - ref).abs()
    print(f"{what}: max|d| = {d.max():.2e}, mean|d| = {d.mean():.2e}")
    assert out.shape == ref.shape and torch.isfinite(out).all()
    assert d.max() < 1e-4 and d.mean() < 1e-5, (what, d.max(), d.mean())


# ------------------------------------------------------------------------------------------------ host, no backend
@pytest.mark.parametrize("T,S", [(100, 2), (100, 7), (100, 10), (100, 37), (100, 99), (100, 100), (1000, 13), (1000, 250), (25, 25), (20, 3)])
def test_timestep_subsequence(T, S):
    tau = GaussianDiffusion(timesteps=T).sampling_timestep_map(S).tolist()
    assert tau == [(2 * k * (T - 1) + (S - 1)) // (2 * (S - 1)) for k in range(S)]
    assert len(tau) == S and tau[0] == 0 and tau[-1] == T - 1 and all(b > a for a, b in zip(tau, tau[1:]))
    assert all(abs(t - k * (T - 1) / (S - 1)) <= 0.5 for k, t in enumerate(tau))
    if S == T:
        assert tau == list(range(T))


@pytest.mark.parametrize("T,S", [(100, 10), (100, 37), (100, 100), (1000, 50), (25, 2)])
@pytest.mark.parametrize("sampler,eta", SOLVERS + [("ddim", 1.0)])
def test_tables_preserve_the_marginals(T, S, sampler, eta):
    """x_k = sqrt(abar_k) x0 + sqrt(1 - abar_k) eps with a constant x0 prediction must give x_{k-1} with abar_{k-1}: the mean identity
    c3 sqrt(abar_k) + c2 + c5 = sqrt(abar_{k-1}) and the variance identity c3^2 (1 - abar_k) + c4^2 = 1 - abar_{k-1} (cN = column N), every
    row, in fp64 (a few ulp of the O(1) terms: 1e-13 covers the cancellation in 1 - abar at small timesteps)"""
    gd = GaussianDiffusion(timesteps=T)
    tau, a, tab = gd._sampler_tables64(S, sampler, eta)
    assert tab.dtype == torch.float64 and tab.shape == (S, 8) and a.dtype == torch.float64
    ap = torch.cat([torch.ones(1, dtype=torch.float64), a[:-1]])
    c2, c3, sg, c5 = tab[:, 2], tab[:, 3], tab[:, 4], tab[:, 5]
    assert (c3 * a.sqrt() + c2 + c5 - ap.sqrt()).abs().max() < 1e-13
    assert (c3 ** 2 * (1 - a) + sg ** 2 - (1 - ap)).abs().max() < 1e-13
    assert torch.equal(tab[:, 0], (1 / a).sqrt()) and torch.equal(tab[:, 1], (1 / a - 1).sqrt())
    assert (tab[:, 6:] == 0).all() and sg[0] == 0
    if sampler != "dpmpp_2m":
        assert (c5 == 0).all()
    else:
        assert (sg == 0).all() and c5[0] == 0 and c5[-1] == 0 and (S < 3 or (c5[1:-1] < 0).all())
        assert tab[0, 2] == 1 and tab[0, 3] == 0
    if sampler == "ddim" and eta is None:
        assert (sg == 0).all()
    tau32, tab32 = gd.sampler_tables(S, sampler, eta)
    assert torch.equal(tau32, tau) and tab32.dtype == torch.float32 and torch.equal(tab32, tab.to(torch.float32))


@pytest.mark.parametrize("T", [25, 100, 1000])
def test_ddpm_on_every_timestep_is_the_reference_table(T):
    """'ddpm' at S = T against sampler_coef_table().  Columns 0..3 (fp64 expressions rounded once, on both sides): at most 1 ulp.  The
    sigma column: the reference's is exp(0.5 * fp32(log variance)) evaluated in fp32 -- the rounding of the logarithm alone moves it by
    sigma * 0.5 * (half a spacing of the logarithm), the fp32 exp and the product by another 1.5 spacings of sigma -- while the rebuilt one
    is the fp64 value rounded once: the difference must stay inside the reference's own error bound"""
    gd = GaussianDiffusion(timesteps=T)
    tau, tab = gd.sampler_tables(T, "ddpm")
    ref = gd.sampler_coef_table()
    assert tau.tolist() == list(range(T))
    sp = lambda v: torch.from_numpy(np.spacing(v.abs().numpy()))
    assert ((tab[:, :4] - ref[:, :4]).abs() <= sp(ref[:, :4])).all(), (tab - ref).abs().max(0)
    bound = 0.25 * ref[:, 4] * sp(gd.posterior_log_variance_clipped.cpu()) + 1.5 * sp(ref[:, 4])
    d = (tab[:, 4] - ref[:, 4]).abs()
    print(f"T = {T}: sigma column max|d| = {d.max():.2e} ({(d / sp(ref[:, 4])).max():.0f} ulp)")
    assert (d <= bound).all() and tab[0, 4] == 0 and (tab[:, 5:] == 0).all()
    assert torch.equal(gd.sampler_tables(T, "ddim", 1.0)[1], tab)


def test_first_dpmpp_step_is_ddim():
    gd = GaussianDiffusion(timesteps=100)
    for S in (2, 10, 37):
        _, _, dd = gd._sampler_tables64(S, "ddim", None)
        _, _, dp = gd._sampler_tables64(S, "dpmpp_2m", None)
        assert (dd[-1] - dp[-1]).abs().max() < 1e-13 and (dd[0] - dp[0]).abs().max() < 1e-13
        if S > 2:
            assert (dd[1:-1, 2] - dp[1:-1, 2]).abs().min() > 1e-4          # the middle rows are second order


def test_dpmpp_2m_rows_from_the_paper():
    """Lu et al. 2022, Algorithm 2, recomputed here from lambda with nothing taken from the code under test but abar: stepping from
    t_prev2 > t_prev > t_cur (rows k+1, k, k-1 of a table that is walked downwards), h_cur = lambda(k-1) - lambda(k), h_prev =
    lambda(k) - lambda(k+1), r = h_prev / h_cur, D = (1 + 1/(2r)) x0(k) - (1/(2r)) x0(k+1),
    x(k-1) = (s(k-1)/s(k)) x(k) - alpha(k-1) (exp(-h_cur) - 1) D.  Pins the split between column 2 and column 5 (the marginal identity only
    sees their sum): an inverted r would fail here"""
    import math
    T, S = 100, 12
    gd = GaussianDiffusion(timesteps=T)
    tau, tab = gd.sampler_tables(S, "dpmpp_2m")
    betas = np.linspace(1000 / T * 1e-4, 1000 / T * 0.02, T, dtype=np.float64)
    abar = np.cumprod(1 - betas)[tau.numpy()]
    lam = [0.5 * math.log(a / (1 - a)) for a in abar]
    for k in range(1, S - 1):                                # the middle rows
        h_cur, h_prev = lam[k - 1] - lam[k], lam[k] - lam[k + 1]
        assert h_cur > 0 and h_prev > 0 and abs(h_prev / h_cur - 1) > 0.02          # uneven spacing in lambda: r and 1/r are told apart
        r = h_prev / h_cur
        m = math.sqrt(abar[k - 1]) * (1 - math.exp(-h_cur))
        want = (m * (1 + 1 / (2 * r)), math.sqrt((1 - abar[k - 1]) / (1 - abar[k])), 0., -m / (2 * r))
        got = tab[k, 2:6].tolist()
        assert all(abs(g - w) <= 2e-7 * max(1., abs(w)) for g, w in zip(got, want)), (k, got, want)          # fp32 rounding of the table
        wrong = -m * r / 2                                   # column 5 with r inverted
        assert abs(got[3] - wrong) > 1e-3 * abs(wrong)


def test_argument_validation():
    """bad values raise before anything is launched (no backend is loaded here: a launch would need one)"""
    im = Imagen([Unet(**TINY), Unet(**TINY, lowres_cond=True)], text_encoder_name="t5_small", image_sizes=[16, 32], timesteps=25, cond_drop_prob=0.15)
    emb, mask = R.synthetic_text(1, length=8, seed=1)
    bad = [dict(sample_steps=1), dict(sample_steps=26), dict(sample_steps=(10,)), dict(sample_steps=(10, 10, 10)), dict(sample_steps=(10, 1)),
           dict(sample_steps=2.5), dict(sample_steps=True), dict(sampler="euler"), dict(sampler="ddpm", sampler_eta=0.5), dict(sampler_eta=0.5),
           dict(sampler="dpmpp_2m", sampler_eta=0.), dict(sampler="ddim", sampler_eta=1.5), dict(sampler="ddim", sampler_eta=-0.1),
           dict(sampler="ddim", sampler_eta="0")]
    for kw in bad:
        with pytest.raises((ValueError, AssertionError)):
            im.sample(text_embeds=emb, text_masks=mask, **kw)
    with pytest.raises(TypeError):
        im.sample(emb, None, None, 1., None, False, None, 10)          # keyword-only
    assert im._parse_solver(None, None, None) == [None, None] and im._parse_solver(25, "ddpm", None) == [None, None]
    assert im._parse_solver((25, 10), None, None) == [None, (10, "ddpm", 1.)]
    assert im._parse_solver(25, "ddim", None) == [(25, "ddim", 0.)] * 2 and im._parse_solver(5, "dpmpp_2m", None) == [(5, "dpmpp_2m", 0.)] * 2
    gd = GaussianDiffusion(timesteps=25)
    for args in ((1, "ddpm"), (26, "ddpm"), (5, "heun"), (5, "ddpm", 0.5), (5, "ddim", 2.)):
        with pytest.raises(ValueError):
            gd.sampler_tables(*args)


# ------------------------------------------------------------------------------------------------ kernels
def _np_history_step(x0, sq, x, prev, z, row):
    """the stated order, one rounding per operation: threshold; mean = c2 x0 + c3 x; mean += c5 prev; x' = mean + c4 z (cN = column N)"""
    f = np.float32
    c2, c3, c4, c5 = f(row[2]), f(row[3]), f(row[4]), f(row[5])
    s = np.where(sq < f(1), f(1), sq).astype(f)[:, None]
    x0c = (np.clip(x0, -s, s) / s).astype(f)
    mean = ((c2 * x0c).astype(f) + (c3 * x).astype(f)).astype(f)
    mean = (mean + (c5 * prev).astype(f)).astype(f)
    return (mean + (c4 * z).astype(f)).astype(f), x0c


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("n", [3 * 16 * 16, 3 * 15 * 15, 27648])
def test_history_tails_bit_exact(backend, n):
    """mi_posterior_ext_fwd with the history term against numpy in the stated operation order, bit for bit (n % 4 != 0 too); x0_prev holds
    the thresholded x0 afterwards; the fused forms (one workgroup per image / cooperating workgroups) give the same bits as the separate
    kernels; without x0_prev the ext entries are the plain ones"""
    dev = setup(backend)
    lib = L.lib()
    B, T, S = 3, 100, 10
    gd = GaussianDiffusion(timesteps=T)
    _, tab = gd.sampler_tables(S, "dpmpp_2m")
    coef = tab.to(dev).contiguous()
    g = torch.Generator().manual_seed(n)
    k_lo, k_hi, w = quantile_rank(n, 0.9)
    st = L.current_stream()
    dv = lambda t: t.clone().to(dev)                          # (a copy on the emulator too: the kernels update in place)
    for k, off in ((5, 0), (S - 1, 0), (3, 2), (0, 0)):
        assert (tab[k, 5] != 0) == (0 < k < S - 1)
        pred2, xt = torch.randn(2 * B, n, generator=g) * 1.5, torch.randn(B, n, generator=g)
        noise, prev0 = torch.randn(S, B, n, generator=g), torch.randn(B, n, generator=g)
        pred2d, noised = pred2.to(dev), noise.to(dev)
        tstate = torch.tensor([k + off], dtype=torch.int32, device=dev)
        # separate kernels: x0 + threshold as ever, then the posterior with history
        x0, s_q = torch.zeros(B, n, device=dev), torch.zeros(B, device=dev)
        hist = torch.zeros(3 * B * 2 * 2048, dtype=torch.int32, device=dev)
        xa, pa = dv(xt), dv(prev0)
        cp = L.MiCfgX0Params(B, n, pred2d.data_ptr(), 1, 3.0, xa.data_ptr(), coef.data_ptr(), tstate.data_ptr(), 0, x0.data_ptr(), 0, off)
        L.check(lib.mi_cfg_x0_fwd(C.byref(cp), st))
        qp = L.MiQuantileParams(B, n, x0.data_ptr(), k_lo, k_hi, w, hist.data_ptr(), s_q.data_ptr(), None)
        L.check(lib.mi_quantile_fwd(C.byref(qp), st))
        pp = L.MiPosteriorParams(B, n, S, x0.data_ptr(), s_q.data_ptr(), xa.data_ptr(), coef.data_ptr(), tstate.data_ptr(), noised.data_ptr(), 0, 0, 0, 0, off)
        ext = L.MiSamplerExtParams(0, pa.data_ptr())
        L.check(lib.mi_posterior_ext_fwd(C.byref(pp), C.byref(ext), st), "mi_posterior_ext_fwd")
        want_x, want_prev = _np_history_step(x0.cpu().numpy(), s_q.cpu().numpy(), xt.numpy(), prev0.numpy(), noise[S - 1 - k].numpy(), tab[k].numpy())
        assert np.array_equal(xa.cpu().numpy().view(np.uint32), want_x.view(np.uint32)), (k, off)
        assert np.array_equal(pa.cpu().numpy().view(np.uint32), want_prev.view(np.uint32)), (k, off)
        if 0 < k < S - 1:
            plain = dv(xt)
            pq = L.MiPosteriorParams.from_buffer_copy(pp)
            pq.x = plain.data_ptr()
            L.check(lib.mi_posterior_ext_fwd(C.byref(pq), C.byref(L.MiSamplerExtParams(0, 0)), st))        # no x0_prev: the plain kernel
            plain2 = dv(xt)
            pq.x = plain2.data_ptr()
            L.check(lib.mi_posterior_fwd(C.byref(pq), st))
            assert torch.equal(plain, plain2) and not torch.equal(plain, xa)
        # the fused forms on the same inputs
        for use_noise in (True, False):
            xs, ps_ = dv(xt), dv(prev0)
            nzp = noised.data_ptr() if use_noise else 0
            if not use_noise:                                  # the on-device generator: the separate kernels again, same (seed, row, stream)
                xa, pa = dv(xt), dv(prev0)
                pr = L.MiPosteriorParams(B, n, S, x0.data_ptr(), s_q.data_ptr(), xa.data_ptr(), coef.data_ptr(), tstate.data_ptr(), 0, 77, 5, 3 << 20, 0, off)
                L.check(lib.mi_posterior_ext_fwd(C.byref(pr), C.byref(L.MiSamplerExtParams(0, pa.data_ptr())), st))
            cf = L.MiCfgX0Params(B, n, pred2d.data_ptr(), 1, 3.0, xs.data_ptr(), coef.data_ptr(), tstate.data_ptr(), 0, 0, 0, off)
            qf = L.MiQuantileParams(B, n, 0, k_lo, k_hi, w, 0, 0, 0, 0, 0)
            pf = L.MiPosteriorParams(B, n, S, 0, 0, xs.data_ptr(), coef.data_ptr(), tstate.data_ptr(), nzp, 77, 5, 3 << 20, 0, off)
            ef = L.MiSamplerExtParams(0, ps_.data_ptr())
            if n <= 16384:
                L.check(lib.mi_sampler_step_small_ext_fwd(C.byref(cf), C.byref(qf), C.byref(pf), C.byref(ef), st), "small ext")
            else:
                assert lib.mi_sampler_group_size(n) == 2
                sync = torch.zeros(lib.mi_sampler_group_sync_bytes(B, n), dtype=torch.uint8, device=dev)
                L.check(lib.mi_sampler_step_group_ext_fwd(C.byref(cf), C.byref(qf), C.byref(pf), C.byref(ef), sync.data_ptr(), st), "group ext")
                assert int(sync[8:12].view(torch.int32).item()) == 0
            assert torch.equal(xs, xa) and torch.equal(ps_, pa), (k, off, use_noise)


@pytest.mark.parametrize("backend", BACKENDS)
def test_mapped_step_kernels(backend):
    dev = setup(backend)
    lib = L.lib()
    tau = GaussianDiffusion(timesteps=100).sampling_timestep_map(12)
    t_map = tau.to(torch.int32).to(dev)
    ext = L.MiSamplerExtParams(t_map.data_ptr(), 0)
    times = torch.zeros(5, dtype=torch.int64, device=dev)
    ts = torch.zeros(1, dtype=torch.int32, device=dev)
    st = L.current_stream()
    L.check(lib.mi_step_set_mapped(ts.data_ptr(), times.data_ptr(), 5, 11, C.byref(ext), st))
    assert ts.item() == 11 and times.tolist() == [99] * 5
    L.check(lib.mi_step_advance_mapped(ts.data_ptr(), times.data_ptr(), 5, C.byref(ext), st))
    assert ts.item() == 10 and times.tolist() == [int(tau[10])] * 5
    L.check(lib.mi_step_advance_by_mapped(ts.data_ptr(), times.data_ptr(), 5, 4, C.byref(ext), st))
    assert ts.item() == 6 and times.tolist() == [int(tau[6])] * 5
    L.check(lib.mi_step_advance_by_mapped(ts.data_ptr(), times.data_ptr(), 5, 6, C.byref(ext), st))
    assert ts.item() == 0 and times.tolist() == [0] * 5
    L.check(lib.mi_step_advance_mapped(ts.data_ptr(), times.data_ptr(), 5, C.byref(ext), st))        # behind the last step: no read outside the map
    assert ts.item() == -1 and times.tolist() == [0] * 5
    assert lib.mi_step_set_mapped(ts.data_ptr(), times.data_ptr(), 5, 3, C.byref(L.MiSamplerExtParams(0, 0)), st) != 0
    assert lib.mi_struct_size(24) == C.sizeof(L.MiSamplerExtParams) == 32 and lib.mi_abi_version() == 12


@pytest.mark.parametrize("backend", BACKENDS)
def test_three_tail_forms_agree_in_the_sampling_loop(backend, monkeypatch):
    """'dpmpp_2m' through the one-workgroup tail, the grouped tail and the separate kernels: identical bits (on-device noise, graphs
    of several steps)"""
    from minimagen_amd import Imagen as IM
    dev = setup(backend)
    gpu = backend == "gpu"
    emb, mask = R.synthetic_text(2, length=10, seed=3)
    for S_img, kinds in ((24, ("small", "separate")), (96 if gpu else 76, ("group", "separate"))):
        outs = {}
        for kind in kinds:
            monkeypatch.setenv("MINIMAGEN_SAMPLER_FUSED", "0" if (kind == "separate" and S_img == 24) else "1")
            monkeypatch.setattr(IM, "SAMPLER_GROUP", 0 if kind == "separate" else 1)
            im, _ = tiny_imagen(S_img, 25, dev)
            outs[kind] = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=2., _seed=11, sample_steps=10, sampler="dpmpp_2m").cpu()
            im.check_device_status()
            sts = next(iter(im.unets[0].engine()._ws.values())).sampler_state
            assert list(sts.keys()) == [(25, 10, "dpmpp_2m", 0.)]
            assert any(hasattr(v, "group_sync") for v in sts.values()) == (kind == "group")
        a, b = (outs[k] for k in kinds)
        assert torch.equal(a, b), kinds
        assert a.isfinite().all() and a.std() > 0.01


@pytest.mark.parametrize("backend", BACKENDS)
def test_deterministic_solvers_ignore_the_step_noise(backend):
    """injected noise: the same x_T with two different streams of step draws gives the same image for 'ddim' (eta 0) and 'dpmpp_2m'
    (their sigma column is 0 -- the draws are still consumed, one per step), a different one for 'ddpm'; another x_T changes all"""
    dev = setup(backend)
    im, _ = tiny_imagen(16, 25, dev)
    emb, mask = R.synthetic_text(2, length=10, seed=3)

    def noise(seed_xt, seed_steps):
        first, rest, calls = R.make_randn(seed_xt), R.make_randn(seed_steps), []
        def fn(shape):
            calls.append(tuple(shape))
            return first(shape) if len(calls) == 1 else rest(shape)
        fn.calls = calls
        return fn

    for sampler, same in (("dpmpp_2m", True), ("ddim", True), ("ddpm", False)):
        kw = dict(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=2., sample_steps=4, sampler=sampler)
        n1 = noise(1, 2)
        a = im.sample(**kw, _noise=n1).clone()
        b = im.sample(**kw, _noise=noise(1, 3)).clone()
        assert len(n1.calls) == 1 + 4                        # x_T, then one draw per step for every solver
        assert torch.equal(a, b) == same, sampler
        assert not torch.equal(a, im.sample(**kw, _noise=noise(5, 2))), sampler


# ------------------------------------------------------------------------------------------------ values against the restated loop
@pytest.mark.parametrize("backend", [pytest.param("emu", marks=pytest.mark.emu)])
@pytest.mark.parametrize("sampler,eta", SOLVERS)
def test_values_emulator(backend, sampler, eta):
    """32^2, B = 2, T = 100, S = 6, cond_scale 3, golden base weights"""
    dev = setup(backend)
    im = make_imagen([32], 100, dev)
    emb, mask = R.synthetic_text(2, length=16, seed=7)
    out = im.sample(text_embeds=emb, text_masks=mask, cond_scale=3., _noise=R.make_randn(3), sample_steps=6, sampler=sampler, sampler_eta=eta)
    ref = restated_sample([I.load("unet0_sd.pt")], [32], 100, 6, sampler, eta, text_embeds=emb, text_masks=mask, cond_scale=3., randn=R.make_randn(3))
    gate(out, ref, f"emulator 32^2 T=100 S=6 {sampler} eta={eta}")


@pytest.mark.parametrize("backend", GPU_ONLY)
@pytest.mark.parametrize("sampler,eta", SOLVERS)
def test_values_base_stage(backend, sampler, eta):
    """base 64^2, cond_scale 3, T = 100, S = 20, B = 2"""
    dev = setup(backend)
    im = make_imagen([64], 100, dev)
    emb, mask = R.synthetic_text(2, length=48, seed=9)
    out = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., _noise=R.make_randn(21), sample_steps=20, sampler=sampler,
                    sampler_eta=eta)
    ref = restated_sample([I.load("unet0_sd.pt")], [64], 100, 20, sampler, eta, text_embeds=emb, text_masks=mask, cond_scale=3., randn=R.make_randn(21))
    gate(out, ref, f"base 64^2 T=100 S=20 {sampler} eta={eta}")
    im.check_device_status()


@pytest.mark.parametrize("backend", GPU_ONLY)
@pytest.mark.parametrize("sampler,eta", [("ddpm", None), ("dpmpp_2m", None)])
def test_values_cascade(backend, sampler, eta):
    """64 -> 256, T = 100, sample_steps = (25, 10), cond_scale 3, B = 2: the grouped tail with history on the 256^2 stage"""
    dev = setup(backend)
    im = make_imagen([64, 256], 100, dev)
    emb, mask = R.synthetic_text(2, length=48, seed=9)
    out = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., _noise=R.make_randn(21), sample_steps=(25, 10), sampler=sampler,
                    sampler_eta=eta)
    ref = restated_sample([I.load("unet0_sd.pt"), I.load("unet1_sd.pt")], [64, 256], 100, (25, 10), sampler, eta, text_embeds=emb, text_masks=mask,
                          cond_scale=3., randn=R.make_randn(21))
    gate(out, ref, f"cascade 64->256 T=100 S=(25, 10) {sampler}")
    im.check_device_status()
    st = [v for u in im.unets for ws in u.engine()._ws.values() for v in ws.sampler_state.values()]
    assert [hasattr(v, "group_sync") for v in st].count(True) == 1


@pytest.mark.parametrize("backend", GPU_ONLY)
def test_values_wide_attention_unet(backend):
    """``Unet()`` default at 64^2 (the wide attention path: its per-step conditioning reads the timestep the mapped step kernels wrote),
    T = 100, S = 8, 'dpmpp_2m' and strided 'ddpm', B = 2, cond_scale 3"""
    dev = setup(backend)
    torch.manual_seed(6)
    u = Unet()
    sd = {k: v.clone() for k, v in u.state_dict().items()}
    im = Imagen((u,), text_encoder_name="t5_small", image_sizes=(64,), timesteps=100, cond_drop_prob=0.1).to(dev).eval()
    emb, mask = R.synthetic_text(2, length=32, seed=7)
    for sampler in ("dpmpp_2m", "ddpm"):
        out = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., _noise=R.make_randn(55), sample_steps=8, sampler=sampler)
        ref = restated_sample([sd], [64], 100, 8, sampler, None, text_embeds=emb, text_masks=mask, cond_scale=3., randn=R.make_randn(55))
        gate(out, ref, f"Unet() default 64^2 T=100 S=8 {sampler}")
    assert next(iter(u.engine()._ws.values())).wide_attn
    im.check_device_status()


# ------------------------------------------------------------------------------------------------ invariants
@pytest.mark.parametrize("backend", BACKENDS)
def test_default_call_is_untouched(backend):
    """sample() == sample(sample_steps=T, sampler='ddpm'), bit for bit, on ONE stage state (the reference's loop: keyed by T alone)"""
    dev = setup(backend)
    gpu = backend == "gpu"
    T = 25 if gpu else 21                                              # (the emulator takes ~1 s per step)
    im = make_imagen([64, 256], T, dev) if gpu else tiny_imagen(16, T, dev)[0]
    emb, mask = R.synthetic_text(2, length=16, seed=7)
    kw = dict(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., _seed=11)
    a = im.sample(**kw).clone()
    b = im.sample(**kw, sample_steps=T, sampler="ddpm").clone()
    assert torch.equal(a, b)
    if gpu:
        assert torch.equal(a, im.sample(**kw, sample_steps=(T, T)))
    for u in im.unets:
        for ws in u.engine()._ws.values():
            assert list(ws.sampler_state.keys()) == [T] and len(ws.sampler_state[T].graphs) == 1
            assert not hasattr(ws.sampler_state[T], "ext")
    im.check_device_status()


@pytest.mark.parametrize("backend,sampler,eta", [pytest.param("gpu", "ddpm", None, marks=pytest.mark.gpu), pytest.param("gpu", "ddim", 0.5, marks=pytest.mark.gpu),
                                                 pytest.param("gpu", "dpmpp_2m", None, marks=pytest.mark.gpu),
                                                 pytest.param("emu", "dpmpp_2m", None, marks=pytest.mark.emu)])
def test_loop_invariants(backend, sampler, eta):
    """graph == eager for S = 7 (one step per graph) and S = 10 (five); the second call replays the cached graph; another seed differs;
    sharded rows == unsharded rows; two solver settings alternating on one Imagen do not disturb each other"""
    dev = setup(backend)
    gpu = backend == "gpu"
    B = 4 if gpu else 2
    im = make_imagen([64], 50, dev) if gpu else tiny_imagen(16, 50, dev)[0]
    emb, mask = R.synthetic_text(B, length=16, seed=7)
    emb, mask = emb.to(dev), mask.to(dev)
    kw = dict(text_embeds=emb, text_masks=mask, cond_scale=3., sampler=sampler, sampler_eta=eta)
    outs = {}
    for S in (7, 10):
        a = outs[S] = im.sample(**kw, _seed=11, sample_steps=S).clone()
        assert torch.equal(a, im.sample(**kw, _seed=11, sample_steps=S, _use_graph=False))
        assert a.isfinite().all() and a.min() >= 0. and a.max() <= 1. and a.std() > 0.01
    kw2 = dict(text_embeds=emb, text_masks=mask, cond_scale=3., _seed=11, sample_steps=10, sampler="ddim" if sampler != "ddim" else "dpmpp_2m")
    other = im.sample(**kw2).clone()
    assert not torch.equal(other, outs[10])
    for S in ((10, 7, 10) if gpu else (7,)):                           # cached graphs, alternating with the other setting
        assert torch.equal(im.sample(**kw, _seed=11, sample_steps=S), outs[S])
        assert torch.equal(im.sample(**kw2), other)
    st = next(iter(im.unets[0].engine()._ws.values())).sampler_state
    graphs = {k: len(v.graphs) for k, v in st.items()}
    assert len(graphs) == 3 and all(n == 1 for n in graphs.values()), graphs          # one state per setting, one cached graph each
    per = {k[1]: next(iter(v.graphs.values()))["per"] for k, v in st.items() if k[2] == sampler}
    assert per == {7: 1, 10: 5}
    assert not torch.equal(im.sample(**kw, _seed=12, sample_steps=10), outs[10])      # the seed is live (x_T at least)
    h = B // 2
    e = im.sample(text_embeds=emb[h:].contiguous(), text_masks=mask[h:].contiguous(), cond_scale=3., sampler=sampler, sampler_eta=eta, _seed=11,
                  _sample_offset=h, sample_steps=10)
    assert torch.equal(e, outs[10][h:])
    if gpu:
        dflt = im.sample(text_embeds=emb, text_masks=mask, cond_scale=3., _seed=11)      # and the default next to them
        assert dflt.isfinite().all() and 50 in st and not torch.equal(dflt, outs[10])
    im.check_device_status()


def test_forwarding_entry_points_pass_the_keywords(tmp_path):
    """generate.sample_and_save(sample_args=) and distributed.sample_distributed(**kwargs) hand the step-count keywords to Imagen.sample
    unchanged (a recording stand-in for the model: no backend needed) and say so in their docstrings"""
    from PIL import Image
    from minimagen_amd import distributed, generate
    seen = []

    class Recorder:
        channels, image_sizes = 3, (8,)

        def sample(self, **kw):
            seen.append(kw)
            if kw.get("return_pil_images"):
                return [Image.new("RGB", (8, 8)) for _ in kw["texts"]]
            return torch.zeros(kw["text_embeds"].shape[0], 3, 8, 8)

        def parameters(self):
            return iter([torch.zeros(1)])

    knobs = dict(sample_steps=(12, 5), sampler="dpmpp_2m")
    generate.sample_and_save(["a", "b"], minimagen=Recorder(), sample_args=dict(cond_scale=3., **knobs), save_directory=str(tmp_path / "out"))
    assert seen[-1]["sample_steps"] == (12, 5) and seen[-1]["sampler"] == "dpmpp_2m" and seen[-1]["cond_scale"] == 3.
    out = distributed.sample_distributed(Recorder(), text_embeds=torch.zeros(3, 4, 16), sample_steps=7, sampler="ddim", sampler_eta=0.25)
    assert out.shape[0] == 3 and seen[-1]["sample_steps"] == 7 and seen[-1]["sampler"] == "ddim" and seen[-1]["sampler_eta"] == 0.25
    assert seen[-1]["_sample_offset"] == 0
    for fn in (generate.sample_and_save, distributed.sample_distributed):
        assert "sample_steps" in fn.__doc__ and "sampler" in fn.__doc__


@pytest.mark.parametrize("backend", BACKENDS)
def test_solver_state_cache_is_bounded(backend, monkeypatch):
    """a caller sweeping sample_steps keeps at most MAX_SOLVER_STATES stage states (tables, graphs) per workspace, least recently used
    out first; an evicted setting is rebuilt to the same bits; the default call's state is never evicted"""
    from minimagen_amd import Imagen as IM
    dev = setup(backend)
    monkeypatch.setattr(IM, "MAX_SOLVER_STATES", 2)
    im, _ = tiny_imagen(16, 25, dev)
    emb, mask = R.synthetic_text(2, length=10, seed=3)
    kw = dict(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=2., _seed=11, sampler="dpmpp_2m")
    ws = lambda: next(iter(im.unets[0].engine()._ws.values()))
    dflt = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=2., _seed=11).clone() if backend == "gpu" else None
    a4 = im.sample(**kw, sample_steps=4).clone()
    im.sample(**kw, sample_steps=3)
    assert torch.equal(im.sample(**kw, sample_steps=4), a4)          # a hit: 4 is now the most recently used
    im.sample(**kw, sample_steps=2)                                    # evicts 3
    keys = [k for k in ws().sampler_state if isinstance(k, tuple)]
    assert [k[1] for k in keys] == [4, 2]
    assert len([k for k in ws().step_tables if len(k) == 3]) == 2
    im.sample(**kw, sample_steps=3)                                    # evicts 4 ...
    assert [k[1] for k in ws().sampler_state if isinstance(k, tuple)] == [2, 3]
    assert torch.equal(im.sample(**kw, sample_steps=4), a4)          # ... which is rebuilt to the same bits
    if dflt is not None:
        assert 25 in ws().sampler_state and torch.equal(im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=2., _seed=11), dflt)
    im.check_device_status()
