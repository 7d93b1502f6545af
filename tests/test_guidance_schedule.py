"""Guidance intervals and schedules of Imagen.sample: argument validation, the interval -> scale table mapping and the
plan on the host; the ABI and the three table-reading launches through the C ABI; the sampling loop -- a stage moving between its B-row
and its 2B-row workspace -- against a restated loop on injected noise (the project's gate: max 1e-4, mean 1e-5); and the invariants of the
loop (equivalences with cond_scale, graphs, lanes, sharding, inpainting, the untouched default call)."""
import ctypes as C
import functools

import pytest
import torch

from minimagen_amd import _lib as L
from minimagen_amd import sampler as S
from minimagen_amd.Imagen import Imagen
from minimagen_amd.Unet import Unet
from minimagen_amd.diffusion_model import GaussianDiffusion
from oracle import resize_restated
from oracle import restated as R
from tests import _inputs as I
from tests._backend import BACKENDS, GPU_ONLY, setup
from tests.test_guidance import EMU_ONLY, _bits, _captions, _sync, run_rescale
from tests.test_sample_steps import TINY, gate, make_imagen, tiny_imagen


# ------------------------------------------------------------------------------------------------ 1. host, no kernel
def test_argument_validation():
    """every bad form raises ValueError before anything is launched (no backend is loaded here: a launch would need one)"""
    im = Imagen([Unet(**TINY), Unet(**TINY)], text_encoder_name="t5_small", image_sizes=[16, 32], timesteps=25, cond_drop_prob=0.15)
    emb, mask = R.synthetic_text(2, length=8, seed=1)
    neg, nmask = R.synthetic_text(2, length=8, seed=2)
    base = dict(text_embeds=emb, text_masks=mask, sample_steps=5)
    ok = dict(base, cond_scale=3.)
    ramp = [1., 2., 3., 4., 5.]
    bad = [dict(ok, guidance_interval=(0.5, 0.25)), dict(ok, guidance_interval=(-0.1, 0.5)), dict(ok, guidance_interval=(0., 1.5)),
           dict(ok, guidance_interval=(0.25,)), dict(ok, guidance_interval=0.5), dict(ok, guidance_interval=(True, 1.)),
           dict(ok, guidance_interval=("0", "1")), dict(ok, guidance_interval=(float("nan"), 1.)),
           dict(ok, guidance_interval=[(0.25, 0.75)]), dict(ok, guidance_interval=[(0.25, 0.75)] * 3),           # one entry per stage
           dict(ok, guidance_interval=[None, None]), dict(ok, guidance_interval=[(0.25, 0.75), 3.]),
           dict(base, guidance_interval=(0.25, 0.75)),                                                            # needs cond_scale != 1
           dict(ok, guidance_schedule=lambda u: 2.),                                                              # the schedule IS the scale
           dict(base, guidance_schedule=[ramp]), dict(base, guidance_schedule=[ramp] * 3), dict(base, guidance_schedule=ramp),
           dict(base, guidance_schedule=[None, None]), dict(base, guidance_schedule=3.),
           dict(base, guidance_schedule=[ramp[:4], None]), dict(base, guidance_schedule=[torch.ones(5, 3), None]),   # lengths and shapes
           dict(base, guidance_schedule=[torch.ones(5, 2, 1), None]), dict(base, guidance_schedule=[torch.ones(2, 5), None]),
           dict(base, guidance_schedule=[[1., float("nan"), 1., 1., 1.], None]), dict(base, guidance_schedule=[[1., float("inf"), 1., 1., 1.], None]),
           dict(base, guidance_schedule=[torch.ones(5, dtype=torch.bool), None]), dict(base, guidance_schedule=["ramp", None]),
           dict(base, guidance_schedule=lambda u: "3"), dict(base, guidance_schedule=lambda u: float("nan")), dict(base, guidance_schedule=lambda u: None),
           # negative prompts and rescale need one guided step
           dict(base, guidance_schedule=lambda u: 1., guidance_rescale=0.5),
           dict(base, guidance_schedule=[[1.] * 5, None], negative_text_embeds=neg, negative_text_masks=nmask),
           dict(ok, guidance_interval=(0.26, 0.49), guidance_rescale=0.5)]                                        # tau = 0 6 12 18 24: no step inside
    for kw in bad:
        with pytest.raises(ValueError):
            im.sample(**kw)
    with pytest.raises(TypeError):
        im.sample(emb, None, None, 3., None, False, None, (0.25, 0.75))           # keyword-only
    solvers = im._parse_solver(5, None, None)
    assert im._parse_guidance_schedule(2, 3., solvers, None, None) is None
    tabs = im._parse_guidance_schedule(2, 3., solvers, [(0.25, 0.75), None], None)
    assert tabs[1] is None and tabs[0].tolist() == [1., 3., 3., 3., 1.]
    tabs = im._parse_guidance_schedule(2, 1., solvers, (0., 0.5), [ramp, torch.tensor([[1., 2.]] * 5)])
    assert tabs[0].tolist() == [1., 1., 3., 4., 5.] and tabs[1].tolist() == [[1., 1.]] * 2 + [[1., 2.]] * 3
    tabs = im._parse_guidance_schedule(2, 1., solvers, None, lambda u: 1. + 3. * (1. - u))                        # a bare callable: every stage
    assert tabs[0].tolist() == tabs[1].tolist() == [1., 1.75, 2.5, 3.25, 4.]
    no_cfg = Imagen([Unet(**TINY)], text_encoder_name="t5_small", image_sizes=[16], timesteps=25, cond_drop_prob=0.)
    with pytest.raises(AssertionError, match="conditional dropout"):
        no_cfg.sample(text_embeds=emb, text_masks=mask, guidance_schedule=[ramp], sample_steps=5)


@pytest.mark.parametrize("T,steps,lo,hi", [(25, 5, 0.25, 0.75), (21, 6, 0.25, 0.75), (25, 25, 0.25, 0.75), (100, 100, 0.25, 0.75), (100, 7, 0., 1.),
                                       (100, 10, 0.5, 0.5), (1000, 13, 0.1, 0.11)])
def test_interval_to_scale_table(T, steps, lo, hi):
    """the step at trained timestep tau_k is guided iff lo (T - 1) <= tau_k <= hi (T - 1), in float64 against the integer tau_k, on
    sampling_timestep_map; entry 0 is the first step executed"""
    tau = GaussianDiffusion(timesteps=T).sampling_timestep_map(steps)
    w = S.guidance_scale_table(tau, T, 2, 3., (lo, hi))
    assert w.shape == (steps,) and w.dtype == torch.float64
    for i in range(steps):
        t = int(tau[steps - 1 - i])
        assert w[i] == (3. if lo * (T - 1) <= t <= hi * (T - 1) else 1.), (i, t)
    if (T, steps) == (25, 5):
        assert w.tolist() == [1., 3., 3., 3., 1.]
    if (T, steps) == (21, 6):
        assert w.tolist() == [1., 1., 3., 3., 1., 1.]
    if (T, steps) == (100, 100):
        assert w.tolist() == [1.] * 25 + [3.] * 50 + [1.] * 25                        # tau 74 .. 25: the middle half
    if (lo, hi) == (0., 1.):
        assert (w == 3.).all()
    per_row = S.guidance_scale_table(tau, T, 2, 1., (lo, hi), torch.full((steps, 2), 5.))
    assert per_row.shape == (steps, 2) and torch.equal(per_row[:, 0], torch.where(w == 3., 5., 1.).double())


def test_plan():
    plan = S.guidance_plan
    assert plan(torch.ones(5)) == [("plain", 0, 5, 1.)]                                              # the cond_scale = 1 call
    assert plan(torch.full((5, 3), 1.)) == [("plain", 0, 5, 1.)]
    assert plan(torch.full((5,), 3.)) == [("scalar", 0, 5, 3.)]                                      # the cond_scale = 3 call
    assert plan(torch.full((5, 2), 0.5)) == [("scalar", 0, 5, 0.5)]
    assert plan(torch.tensor([7.3] * 4, dtype=torch.float64)) == [("scalar", 0, 4, 7.3)]             # the caller's value, not its fp32 rounding
    assert plan(torch.tensor([1., 3., 3., 3., 1.])) == [("plain", 0, 1, 1.), ("scalar", 1, 4, 3.), ("plain", 4, 5, 1.)]
    assert plan(torch.tensor([1., 1., 3., 3., 1., 1.])) == [("plain", 0, 2, 1.), ("scalar", 2, 4, 3.), ("plain", 4, 6, 1.)]
    assert plan(torch.tensor([3., 1., 3.])) == [("scalar", 0, 1, 3.), ("plain", 1, 2, 1.), ("scalar", 2, 3, 3.)]
    assert plan(torch.tensor([1., 2., 3., 4.])) == [("plain", 0, 1, 1.), ("table", 1, 4, None)]
    assert plan(torch.tensor([2., 3., 3., 1.])) == [("table", 0, 3, None), ("plain", 3, 4, 1.)]      # one value on some steps only: still a table
    assert plan(torch.tensor([[1., 1.], [3., 1.], [3., 3.]])) == [("plain", 0, 1, 1.), ("table", 1, 3, None)]     # a row at 1 beside a 3
    assert plan(torch.tensor([[3., 3.], [3., 3.], [1., 1.]])) == [("scalar", 0, 2, 3.), ("plain", 2, 3, 1.)]
    assert plan(torch.tensor([[2., 4.]] * 3)) == [("table", 0, 3, None)]


def test_forwarding_entry_points_pass_the_keywords(tmp_path, monkeypatch):
    """generate.sample_and_save(sample_args=) and distributed.sample_distributed(**kwargs) hand the two keywords to Imagen.sample (a recording
    stand-in for the model), an [S, B] schedule sharded along dimension 1 by the captions' row bounds, and say so"""
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

    f = lambda u: 2.
    generate.sample_and_save(["a", "b"], minimagen=Recorder(), sample_args=dict(cond_scale=3., guidance_interval=(0.25, 0.75)), save_directory=str(tmp_path / "a"))
    assert seen[-1]["guidance_interval"] == (0.25, 0.75) and seen[-1]["cond_scale"] == 3.
    generate.sample_and_save(["a", "b"], minimagen=Recorder(), sample_args=dict(guidance_schedule=f), save_directory=str(tmp_path / "b"))
    assert seen[-1]["guidance_schedule"] is f
    per_row, uniform = torch.arange(12.).reshape(4, 3), [1., 2., 3., 4.]
    text = dict(text_embeds=torch.zeros(3, 4, 16), text_masks=torch.ones(3, 4, dtype=torch.bool))
    out = distributed.sample_distributed(Recorder(), **text, guidance_interval=(0., 0.5), guidance_schedule=[per_row])
    assert out.shape[0] == 3 and seen[-1]["guidance_interval"] == (0., 0.5) and torch.equal(seen[-1]["guidance_schedule"][0], per_row)
    monkeypatch.setattr(distributed.dist, "is_initialized", lambda: True)
    monkeypatch.setattr(distributed.dist, "get_world_size", lambda group=None: 2)
    monkeypatch.setattr(distributed.dist, "get_rank", lambda group=None: 1)
    lo, hi = distributed.shard_bounds(3, 2, 1)
    assert (lo, hi) == (2, 3)
    sched = [per_row, None, uniform, f, per_row.tolist()]
    distributed.sample_distributed(Recorder(), **text, guidance_schedule=sched, gather=False)
    got = seen[-1]["guidance_schedule"]
    assert seen[-1]["_sample_offset"] == lo and torch.equal(got[0], per_row[:, lo:hi]) and got[1] is None and got[2] == uniform and got[3] is f
    assert torch.equal(torch.as_tensor(got[4]), per_row[:, lo:hi])
    assert torch.equal(sched[0], per_row) and len(sched) == 5                                    # the caller's list is not written
    distributed.sample_distributed(Recorder(), **text, guidance_schedule=f, gather=False)
    assert seen[-1]["guidance_schedule"] is f
    for fn in (generate.sample_and_save, distributed.sample_distributed):
        assert "guidance_interval" in fn.__doc__ and "guidance_schedule" in fn.__doc__


# ------------------------------------------------------------------------------------------------ 2. the ABI and the launches
@pytest.mark.parametrize("backend", BACKENDS)
def test_abi_is_additive(backend):
    setup(backend)
    lib = L.lib()
    assert lib.mi_abi_version() == 12
    assert lib.mi_struct_size(34) == C.sizeof(L.MiCfgSchedParams) == 48
    assert lib.mi_struct_size(33) == C.sizeof(L.MiCfgRescaleParams) == 32
    assert lib.mi_struct_size(30) == -1
    for name in ("mi_cfg_sched_combine_fwd", "mi_cfg_sched_rescale_stats_fwd", "mi_cfg_sched_rescale_apply_fwd"):
        getattr(lib, name)


KERNEL_CASES = [(1, 192), (2, 12288), (3, 4099), (2, 196608)]
T_STATE, T_OFF, ROWS = 2, 1, 3            # the launches address table row T_STATE - T_OFF = 1; the other rows hold NaN


def _table(scales, dev):
    tab = torch.full((ROWS, len(scales)), float("nan"))
    tab[T_STATE - T_OFF] = torch.tensor(scales)
    return tab.contiguous().to(dev)


def _inputs(B, n):
    gen = torch.Generator().manual_seed(100 + n % 97)
    return torch.randn(B, n, generator=gen) * 0.8 + 0.1, torch.randn(B, n, generator=gen) * 0.7 - 0.05


def run_sched(backend, dev, c, u, scales, phi=None):
    """the combine launch (phi None) or the two sched rescale launches -> (pred2 [2B, n], partials [B, chunks, 4]), on the host"""
    lib = L.lib()
    B, n = c.shape
    pred2 = torch.cat((c, u)).contiguous().to(dev)
    tab, t_state = _table(scales, dev), torch.tensor([T_STATE], dtype=torch.int32).to(dev)
    part = torch.zeros(B, lib.mi_cfg_rescale_chunks(n), 4, dtype=torch.float64, device=dev)
    p = L.MiCfgSchedParams(B, n, pred2.data_ptr(), tab.data_ptr(), t_state.data_ptr(), T_OFF, phi or 0., part.data_ptr() if phi is not None else 0)
    if phi is None:
        L.check(lib.mi_cfg_sched_combine_fwd(C.byref(p), L.current_stream()), "mi_cfg_sched_combine_fwd")
    else:
        L.check(lib.mi_cfg_sched_rescale_stats_fwd(C.byref(p), L.current_stream()), "mi_cfg_sched_rescale_stats_fwd")
        L.check(lib.mi_cfg_sched_rescale_apply_fwd(C.byref(p), L.current_stream()), "mi_cfg_sched_rescale_apply_fwd")
    _sync(backend)
    return pred2.cpu(), part.cpu()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("B,n", KERNEL_CASES)
def test_combine_kernel_bits(backend, B, n):
    """less than one chunk | whole chunks (the base image) | odd n across a chunk boundary (the element path) | many chunks (the SR image):
    u + (c - u) s in separate fp32 torch ops, to the bit; a row at s = 1 keeps c to the bit; the null rows are untouched"""
    dev = setup(backend)
    c, u = _inputs(B, n)
    scales = [3.0, 1.0, 0.37][:B] if B > 1 else [7.5]
    out, _ = run_sched(backend, dev, c, u, scales)
    for b, s in enumerate(scales):
        want = c[b] if s == 1. else u[b] + (c[b] - u[b]) * torch.tensor(s, dtype=torch.float32)
        assert torch.equal(_bits(out[b]), _bits(want)), (b, s)
    assert torch.equal(_bits(out[B:]), _bits(u))
    ones, _ = run_sched(backend, dev, c, u, [1.0] * B)
    assert torch.equal(_bits(ones), _bits(torch.cat((c, u))))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("B,n", KERNEL_CASES)
def test_sched_rescale_kernels_are_the_scalar_entries(backend, B, n):
    """a constant table: the bits of mi_cfg_rescale_stats_fwd / _apply_fwd, output and partials both; per-row scales: every image is the
    scalar entry run on that image alone"""
    dev = setup(backend)
    c, u = _inputs(B, n)
    out, part = run_sched(backend, dev, c, u, [3.0] * B, phi=0.7)
    ref, ref_part = run_rescale(backend, dev, c, u, 3.0, 0.7)
    assert torch.equal(_bits(out), _bits(ref)) and torch.equal(part.view(torch.int64), ref_part.view(torch.int64))
    scales = [7.5, 0.5, 1.0][:B]
    out, part = run_sched(backend, dev, c, u, scales, phi=0.3)
    for b, s in enumerate(scales):
        ref, ref_part = run_rescale(backend, dev, c[b:b + 1], u[b:b + 1], s, 0.3)
        assert torch.equal(_bits(out[b]), _bits(ref[0])) and torch.equal(part[b].view(torch.int64), ref_part[0].view(torch.int64)), (b, s)
    assert torch.equal(_bits(out[B:]), _bits(u))


@pytest.mark.parametrize("backend", BACKENDS)
def test_sched_kernels_reject_bad_arguments(backend):
    dev = setup(backend)
    lib = L.lib()
    pred2, part = torch.zeros(2, 64, device=dev), torch.zeros(1, 1, 4, dtype=torch.float64, device=dev)
    tab, t_state = torch.full((3, 1), 3.0, device=dev), torch.tensor([2], dtype=torch.int32).to(dev)
    good = (1, 64, pred2.data_ptr(), tab.data_ptr(), t_state.data_ptr(), 1, 0.5, part.data_ptr())
    fns = (lib.mi_cfg_sched_combine_fwd, lib.mi_cfg_sched_rescale_stats_fwd, lib.mi_cfg_sched_rescale_apply_fwd)
    for k, v in ((0, 0), (0, -1), (0, 70000), (1, 0), (1, -4), (2, 0), (3, 0), (4, 0), (5, -1), (6, 1.5), (6, -0.5), (6, float("nan"))):
        args = list(good)
        args[k] = v
        for fn in fns:
            assert fn(C.byref(L.MiCfgSchedParams(*args)), L.current_stream()) == -1, (k, v)
    for fn in fns[1:]:                                                         # the rescale forms need their partials
        assert fn(C.byref(L.MiCfgSchedParams(*good[:7], 0)), L.current_stream()) == -1
    for fn in fns:
        assert fn(None, L.current_stream()) == -1
    _sync(backend)
    assert (pred2 == 0).all() and (part == 0).all()


# ------------------------------------------------------------------------------------------------ 3. the loop against a restated loop
def restated_scheduled_sample(sds, sizes, T, steps, sampler, *, text_embeds, text_masks, scales, randn, negative=None, phi=0.,
                              lowres_sample_noise_level=0.2):
    """tests.test_guidance.restated_guided_sample with the scale per step: ``scales`` = per stage a tensor [S] or [S, B] in execution order.
    ONE R.unet_forward where every row's scale is 1 (no negative captions, no rescale there), two forwards combined per row otherwise."""
    b = text_embeds.shape[0]
    lowres_sched = R.Schedule(T)
    img = None
    for sd, size, S_, w in zip(sds, sizes, steps, scales):
        kw = {}
        if "to_lowres_time_hiddens.1.weight" in sd:
            lt = lowres_sched.get_times(b, lowres_sample_noise_level)
            low = resize_restated.resize(img, scale_factors=size / img.shape[-1], pad_mode='reflect') if img.shape[-1] != size else img
            low = lowres_sched.q_sample(low, int(lt[0]), randn(low.shape))
            kw.update(lowres_cond_img=low * 2 - 1, lowres_noise_times=lt)
        tau, tab = GaussianDiffusion(timesteps=T).sampler_tables(S_, sampler, None)
        w = torch.as_tensor(w, dtype=torch.float32).reshape(S_, -1).expand(S_, b)
        shape = (b, 3, size, size)
        x, prev = randn(shape), torch.zeros(shape)
        for k in range(S_ - 1, -1, -1):
            t = torch.full((b,), int(tau[k]), dtype=torch.long)
            s_row = w[S_ - 1 - k]
            pred = R.unet_forward(sd, x, t, text_embeds=text_embeds, text_mask=text_masks, cond_drop_prob=0., **kw)
            if (s_row != 1.).any():
                pos = pred
                if negative is None:
                    neg = R.unet_forward(sd, x, t, text_embeds=text_embeds, text_mask=text_masks, cond_drop_prob=1., **kw)
                else:
                    neg = R.unet_forward(sd, x, t, text_embeds=negative[0], text_mask=negative[1], cond_drop_prob=0., **kw)
                pred = neg + (pos - neg) * s_row.reshape(b, 1, 1, 1)
                if phi:
                    sp, sg = pos.double().flatten(1).std(dim=1, unbiased=False), pred.double().flatten(1).std(dim=1, unbiased=False)
                    pred = (pred.double() * (phi * sp / sg + (1. - phi)).reshape(b, 1, 1, 1)).float()
            x0 = tab[k, 0] * x - tab[k, 1] * pred
            s, *_ = R.dynamic_threshold_quantile(x0.reshape(b, -1).abs(), 0.9)
            s = s.clamp(min=1.).reshape(b, 1, 1, 1)
            x0 = x0.clamp(-s, s) / s
            z = randn(shape)
            x = ((tab[k, 2] * x0 + tab[k, 3] * x) + tab[k, 5] * prev) + tab[k, 4] * z
            prev = x0
        img = (x.clamp(-1., 1.) + 1) * 0.5
    return img


NOISE = 21
RAMP = torch.stack((torch.linspace(1., 4., 5), torch.tensor([1., 1., 2.5, 1., 3.5])), dim=1)     # [S, B]: row 0 ramps 1 -> 4, row 1 goes back to 1 inside


@functools.lru_cache(maxsize=None)
def _reference(which, sampler, form):
    """one restated run per (model, sampler, form), shared by the tests that need it: -> (reference image, the always-guided image)"""
    if which == "tiny":
        torch_dev = torch.device("cpu")
        sds, sizes, T, steps = [tiny_imagen(16, 21, torch_dev)[1]], [16], 21, (6,)
        emb, mask, neg, nmask = _captions(12, 7)
    else:
        sds = [I.load("unet0_sd.pt")] + ([I.load("unet1_sd.pt")] if which == "cascade" else [])
        sizes, T, steps = ([64, 256] if which == "cascade" else [64]), 25, ((5, 5) if which == "cascade" else (5,))
        emb, mask, neg, nmask = _captions(48, 20)
    guided = [torch.full((s,), 3.) for s in steps]
    scales, phi, negative = {"interval": ([torch.tensor([1., 1., 3., 3., 1., 1.])] if which == "tiny" else [torch.tensor([1., 3., 3., 3., 1.])] * len(steps), 0., None),
                             "ramp": ([RAMP], 0., None),
                             "ramp+rescale+negatives": ([RAMP], 0.7, (neg, nmask))}[form]
    if form.startswith("ramp"):
        guided = [torch.full((5,), 4.)]
    run = lambda w: restated_scheduled_sample(sds, sizes, T, steps, sampler, text_embeds=emb, text_masks=mask, scales=w, randn=R.make_randn(NOISE),
                                              negative=negative, phi=phi)
    return run(scales), run(guided)


def _check_against_reference(out, which, sampler, form, what):
    """the gate against the restated loop -- and that loop really differs from the always-guided one by 100 x the gate, so the gate tells them apart"""
    ref, always = _reference(which, sampler, form)
    d = (ref - always).abs()
    print(f"{what}: restated vs always guided: max|d| = {d.max():.2e}, mean|d| = {d.mean():.2e}")
    assert d.max() >= 1e-2 and d.mean() >= 1e-3, (what, d.max(), d.mean())
    gate(out, ref, what)


def _two_workspaces(eng, B):
    """the stage really holds a B-row and a 2B-row workspace"""
    rows = sorted(ws.B2 for ws in eng._ws.values())
    assert rows == [B, 2 * B], rows
    return {ws.B2: (key, ws) for key, ws in eng._ws.items()}


@pytest.mark.parametrize("backend", EMU_ONLY)
def test_values_emulator(backend):
    """tiny U-Net at 16^2, T = 21 (at T = 20 the schedule has abar_T = 0), S = 6, B = 2, interval (0.25, 0.75): tau = 20 16 12 8 4 0, the scales
    [1, 1, 3, 3, 1, 1] -- plain, a guided run, plain; two hand-overs"""
    dev = setup(backend)
    im, _ = tiny_imagen(16, 21, dev)
    emb, mask, _, _ = _captions(12, 7)
    out = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., _noise=R.make_randn(NOISE), sample_steps=6, guidance_interval=(0.25, 0.75))
    im.check_device_status()
    _check_against_reference(out, "tiny", "ddpm", "interval", "emulator 16^2 T=21 S=6 interval (0.25, 0.75)")
    _two_workspaces(im.unets[0].engine(), 2)


FORMS = {"interval": dict(cond_scale=3., guidance_interval=(0.25, 0.75)),
         "ramp": dict(guidance_schedule=[RAMP]),
         "ramp+rescale+negatives": dict(guidance_schedule=[RAMP], guidance_rescale=0.7)}


@pytest.mark.parametrize("backend", GPU_ONLY)
@pytest.mark.parametrize("sampler", ["ddpm", "dpmpp_2m"])
@pytest.mark.parametrize("form", list(FORMS))
def test_values_base_stage(backend, sampler, form):
    """the golden base U-Net at 64^2, T = 25, S = 5, B = 2.  The interval: plain, 3 guided steps, plain -- two hand-overs, and the dpmpp_2m history
    crosses both.  The ramp 1 -> 4 with per-row columns: a plain step, then a table run (mi_cfg_sched_combine_fwd; a row back at 1 inside it).
    The third form adds phi = 0.7 and negative captions to the ramp: the table run goes through mi_cfg_sched_rescale_stats_fwd / _apply_fwd,
    which no other loop test reaches.  (On the interval, phi = 0.7 pulls the guided steps towards the conditional prediction: the restated
    loop is then only 9.99e-3 max / 1.19e-3 mean (ddpm), 7.98e-3 / 1.03e-3 (dpmpp_2m) from the always-guided one, measured on the CPU --
    too close to 100 x the gate to tell the two apart, so that combination is not a case here.)"""
    dev = setup(backend)
    im = make_imagen([64], 25, dev)
    emb, mask, neg, nmask = _captions(48, 20)
    kw = dict(FORMS[form])
    if "negatives" in form:
        kw.update(negative_text_embeds=neg.to(dev), negative_text_masks=nmask.to(dev))
    out = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), _noise=R.make_randn(NOISE), sample_steps=5, sampler=sampler, **kw)
    im.check_device_status()
    _check_against_reference(out, "base", sampler, form, f"base 64^2 T=25 S=5 {sampler} {form}")
    by_rows = _two_workspaces(im.unets[0].engine(), 2)
    key, ws = by_rows[4]
    (st,) = ws.sampler_state.values()
    assert (key[-1] == "nofold") == (form != "interval") and (st.scale_tab is not None) == (form != "interval")
    assert (st.rescale_partials is not None) == ("rescale" in form)
    if form != "interval":
        assert torch.equal(st.scale_tab.cpu(), RAMP.flip(0))                          # row k: the step at index k


@pytest.mark.parametrize("backend", GPU_ONLY)
def test_values_cascade(backend):
    """64 -> 256, T = 25, S = (5, 5), B = 2, the interval on both stages: the SR stage's guided run is on the FOLDED workspace, the grouped tail
    runs on both of its workspaces, and the low-resolution image is drawn once and copied"""
    dev = setup(backend)
    im = make_imagen([64, 256], 25, dev)
    emb, mask, _, _ = _captions(48, 20)
    out = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., _noise=R.make_randn(NOISE), sample_steps=(5, 5), guidance_interval=(0.25, 0.75))
    im.check_device_status()
    _check_against_reference(out, "cascade", "ddpm", "interval", "cascade 64->256 T=25 S=(5, 5) interval")
    _two_workspaces(im.unets[0].engine(), 2)
    by_rows = _two_workspaces(im.unets[1].engine(), 2)
    assert by_rows[4][1].cfg_fold is not None and "nofold" not in by_rows[4][0] and by_rows[2][1].cfg_fold is None
    for _, ws in by_rows.values():
        (st,) = ws.sampler_state.values()
        assert hasattr(st, "group_sync")
    assert torch.equal(by_rows[2][1].lowres, by_rows[4][1].lowres)


# ------------------------------------------------------------------------------------------------ 4. equivalences, graphs, lanes, sharding
def _keys(im):
    return [(k, sk, tuple(st.graphs)) for u in im.unets for k, ws in u.engine()._ws.items() for sk, st in ws.sampler_state.items()]


@pytest.mark.parametrize("backend", GPU_ONLY)
def test_equivalences_with_cond_scale(backend):
    """interval (0, 1) or a constant schedule s IS cond_scale = s, an all-ones schedule IS cond_scale = 1: the bits, and no new workspace, state
    or graph key"""
    dev = setup(backend)
    im = make_imagen([64], 25, dev)
    emb, mask = R.synthetic_text(2, length=16, seed=7)
    kw = dict(text_embeds=emb.to(dev), text_masks=mask.to(dev), _seed=11, sample_steps=5)
    guided, plain = im.sample(**kw, cond_scale=3.).clone(), im.sample(**kw).clone()
    before = _keys(im)
    assert len(before) == 2 and not torch.equal(guided, plain)
    assert torch.equal(im.sample(**kw, cond_scale=3., guidance_interval=(0., 1.)), guided)
    assert torch.equal(im.sample(**kw, guidance_schedule=lambda u: 3.), guided)
    assert torch.equal(im.sample(**kw, guidance_schedule=[torch.full((5, 2), 3.)]), guided)
    assert torch.equal(im.sample(**kw, guidance_schedule=[[1.] * 5]), plain)
    assert torch.equal(im.sample(**kw, guidance_schedule=lambda u: 1.), plain)
    assert torch.equal(im.sample(**kw, cond_scale=3., guidance_interval=(0., 1.), guidance_rescale=0.7), im.sample(**kw, cond_scale=3., guidance_rescale=0.7))
    assert [k for k in _keys(im) if "nofold" not in k[0]] == before
    im.check_device_status()


@pytest.mark.parametrize("backend", GPU_ONLY)
def test_graphs_lanes_and_other_values(backend):
    """graph replay == eager execution; a second call with other table values replays the same graphs and gives another image; two _async
    calls (one per lane) equal the synchronous result"""
    dev = setup(backend)
    im = make_imagen([64], 25, dev)
    emb, mask = R.synthetic_text(2, length=16, seed=7)
    kw = dict(text_embeds=emb.to(dev), text_masks=mask.to(dev), _seed=11, sample_steps=7, sampler="dpmpp_2m")
    ramp = [torch.linspace(1., 4., 7)]
    a = im.sample(**kw, guidance_schedule=ramp).clone()
    keys = _keys(im)
    # the plain step is one graph of 1 step; the 6-step table run replays a graph of 5 and one of 1: their keys carry the marker and the length
    tab_graphs = [g for k, _, g in keys if k[1] == 4][0]
    assert sorted(k[-1] for k in tab_graphs) == [("len", 1), ("len", 5)] and all(k[-2] == "sched" for k in tab_graphs)
    assert torch.equal(im.sample(**kw, guidance_schedule=ramp, _use_graph=False), a)
    b = im.sample(**kw, guidance_schedule=[torch.linspace(1., 2., 7)]).clone()
    assert _keys(im) == keys and not torch.equal(a, b) and b.isfinite().all()
    assert torch.equal(im.sample(**kw, guidance_schedule=ramp), a)
    iv = im.sample(**kw, cond_scale=3., guidance_interval=(0.25, 0.75)).clone()
    assert torch.equal(im.sample(**kw, cond_scale=3., guidance_interval=(0.25, 0.75), _use_graph=False), iv)
    outs = [im.sample(**kw, cond_scale=3., guidance_interval=(0.25, 0.75), _async=True) for _ in range(2)]
    outs += [im.sample(**kw, guidance_schedule=ramp, _async=True) for _ in range(2)]
    im.wait_pending_samples()
    torch.cuda.synchronize()
    assert all(torch.equal(o, iv) for o in outs[:2]) and all(torch.equal(o, a) for o in outs[2:])
    im.check_device_status()


@pytest.mark.parametrize("backend", GPU_ONLY)
def test_sharding(backend):
    """a row-uniform schedule: the sharded rows are the unsharded rows to the bit; per-row schedules whose shards take different plans (a shard
    whose rows are all 1 on a step runs it unguided): within the gate, and whether the bits agreed is printed"""
    dev = setup(backend)
    im = make_imagen([64], 25, dev)
    B, h = 4, 2
    emb, mask = R.synthetic_text(B, length=16, seed=7)
    emb, mask = emb.to(dev), mask.to(dev)
    kw = dict(_seed=11, sample_steps=5)
    shard = lambda sched, lo, hi: im.sample(text_embeds=emb[lo:hi].contiguous(), text_masks=mask[lo:hi].contiguous(), _sample_offset=lo,
                                            guidance_schedule=[sched if sched.dim() == 1 else sched[:, lo:hi]], **kw)
    uniform = torch.tensor([1., 1., 2., 3., 4.])
    full = im.sample(text_embeds=emb, text_masks=mask, guidance_schedule=[uniform], **kw).clone()
    assert torch.equal(torch.cat((shard(uniform, 0, h).clone(), shard(uniform, h, B))), full)
    per_row = torch.tensor([[1., 1., 1., 1.], [1., 1., 2., 3.], [2., 2., 3., 1.], [3., 3., 1., 1.], [1., 1., 4., 4.]])
    full = im.sample(text_embeds=emb, text_masks=mask, guidance_schedule=[per_row], **kw).clone()
    parts = torch.cat((shard(per_row, 0, h).clone(), shard(per_row, h, B)))
    print(f"per-row schedule, sharded vs unsharded across different plans: bits agree = {torch.equal(parts, full)}")
    gate(parts, full.cpu(), "per-row schedule, sharded vs unsharded")
    im.check_device_status()


@pytest.mark.parametrize("backend", GPU_ONLY)
def test_inpainting_through_a_handover_returns_the_known_pixels(backend):
    """a full mask through plain -> guided -> plain (every workspace holds the known image and mask): the known image within 2^-22"""
    dev = setup(backend)
    im = make_imagen([64], 25, dev)
    emb, mask, _, _ = _captions(16, 9)
    y = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(3))
    for kw in (dict(cond_scale=3., guidance_interval=(0.25, 0.75)), dict(guidance_schedule=[RAMP])):
        out = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), _seed=11, sample_steps=5, inpaint_images=y.to(dev),
                        inpaint_masks=torch.ones(2, 1, 64, 64, device=dev), **kw).cpu()
        d = (out - y).abs().max().item()
        print(f"full mask through a hand-over {sorted(kw)}: max|d| = {d:.3e}")
        assert d <= 2. ** -22
    im.check_device_status()


@pytest.mark.parametrize("backend", GPU_ONLY)
def test_default_call_is_untouched(backend):
    """sample() before and after interval and schedule calls: the same keys on its workspaces and the same bits"""
    dev = setup(backend)
    T = 25
    im = make_imagen([64, 256], T, dev)
    emb, mask = R.synthetic_text(2, length=16, seed=7)
    kw = dict(text_embeds=emb.to(dev), text_masks=mask.to(dev), _seed=11)
    a = im.sample(**kw, cond_scale=3.).clone()
    before = _keys(im)
    assert len(before) == 2 and all(sk == T and len(g) == 1 for k, sk, g in before)
    for off in (dict(guidance_interval=None), dict(guidance_schedule=None)):
        assert torch.equal(im.sample(**kw, cond_scale=3., **off), a)
    assert _keys(im) == before
    iv = im.sample(**kw, cond_scale=3., guidance_interval=(0.25, 0.75)).clone()
    assert not torch.equal(iv, a) and iv.isfinite().all()
    after = _keys(im)
    # the guided runs went through the default call's workspaces and states: its graph is still there, first, beside the runs' own
    guided_after = [(k, sk, g) for k, sk, g in after if k[1] == 4]
    assert [(k, sk) for k, sk, _ in guided_after] == [(k, sk) for k, sk, _ in before]
    assert all(g[0] == g0[0] and all(key[-1][0] == "len" for key in g[1:]) for (_, _, g), (_, _, g0) in zip(guided_after, before))
    assert torch.equal(im.sample(**kw, cond_scale=3.), a) and _keys(im) == after
    im.check_device_status()
