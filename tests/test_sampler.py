"""Imagen.sample through the HIP-graph sampler: parity with the reference's golden outputs (injected noise),
determinism, graph == eager, and the data-parallel sharding property (bit-identical rows)."""
import pytest
import torch

from minimagen_amd import _lib as L
from minimagen_amd.Imagen import Imagen
from minimagen_amd.Unet import Unet
from minimagen_amd.sample_call import StageCall
from oracle import restated as R
from tests import _inputs as I
from tests._backend import BACKENDS, GPU_ONLY, setup


def make_imagen(sizes, T, dev, cond_drop_prob=0.15):
    p = I.unet_params()
    unets = [Unet(**p["unet0"])] + [Unet(**p["unet1"]) for _ in sizes[1:]]      # every SR stage uses the unet_1 parameters
    im = Imagen(unets, text_encoder_name="t5_small", image_sizes=sizes, timesteps=T, cond_drop_prob=cond_drop_prob)
    im.unets[0].load_state_dict(I.load("unet0_sd.pt"))
    for u in im.unets[1:]:
        u.load_state_dict(I.load("unet1_sd.pt"))
    return im.to(dev)


CASES = [pytest.param("sample_base_cs3.pt", "emu", marks=pytest.mark.emu)] + \
        [pytest.param(n, "gpu", marks=pytest.mark.gpu) for n in ("sample_base_cs1.pt", "sample_base_cs3.pt", "sample_cascade.pt")]


@pytest.mark.parametrize("name,backend", CASES)
def test_sample_matches_reference_golden(name, backend):
    """full cascade, max|d| <= 1e-4 and mean|d| <= 1e-5 on [0,1] images"""
    dev = setup(backend)
    g = I.load(name); m = g["meta"]
    im = make_imagen(m["sizes"], m["T"], dev)
    emb, mask = I.text(m)
    out = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=m["cond_scale"], _noise=R.make_randn(m["noise_seed"]))
    d = (out.cpu() - g["out"]).abs()
    assert out.shape == g["out"].shape and d.max() < 1e-4 and d.mean() < 1e-5, (d.max(), d.mean())


@pytest.mark.parametrize("backend", GPU_ONLY)
@pytest.mark.parametrize("name", ["sample_base_cs3.pt", "sample_cascade.pt"])
def test_sample_half_precision_golden(name, backend):
    """BASELINE's reduced-precision configurations (single fp16 term on the matrix cores; fp32 accumulate, softmax, statistics,
    storage): SURVEY.md 8(c) half-precision gate max|d| <= 3e-2, mean|d| <= 3e-3 on [0,1] images vs the fp32 reference"""
    dev = setup(backend)
    g = I.load(name); m = g["meta"]
    im = make_imagen(m["sizes"], m["T"], dev)
    emb, mask = I.text(m)
    out = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=m["cond_scale"], _noise=R.make_randn(m["noise_seed"]), _precision="half")
    d = (out.cpu() - g["out"]).abs()
    assert d.max() < 3e-2 and d.mean() < 3e-3, (d.max(), d.mean())
    assert d.max() > 2e-6                                              # the reduced-precision kernels really ran
    out32 = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=m["cond_scale"], _noise=R.make_randn(m["noise_seed"]))
    assert (out32.cpu() - g["out"]).abs().max() < 1e-4                  # and the default stays fp32-grade


@pytest.mark.parametrize("backend", GPU_ONLY)
def test_step_golden(backend):
    """one _p_sample step (Imagen.py:329-370) through the HIP kernels exactly as Imagen._p_sample_loop wires them --
    U-Net (2B rows) -> mi_cfg_x0_fwd -> mi_quantile_fwd -> mi_posterior_fwd with injected noise -- vs the reference's x_{t-1} (t=13 and t=0)"""
    import ctypes as C
    from minimagen_amd import _lib as L
    from minimagen_amd.helpers import quantile_rank
    dev = setup(backend)
    lib = L.lib()
    g = I.load("step.pt"); m = g["meta"]
    emb, mask = I.text(m)
    im = make_imagen([64], m["T"], dev)
    unet, sched, T = im.unets[0], im.noise_schedulers[0], m["T"]
    B, n = 2, 3 * 64 * 64
    for t, st in g["steps"].items():
        x = I.seeded((B, 3, 64, 64), st["x_seed"])
        noise = R.make_randn(st["noise_seed"])((B, 3, 64, 64))
        pred = unet.forward_with_cond_scale(x.to(dev), torch.full((B,), t).to(dev), text_embeds=emb.to(dev), text_mask=mask.to(dev), cond_scale=3.)
        assert (pred.cpu() - st["pred"]).abs().max() < 6e-5
        # the sampler step itself: same launch sequence as Imagen._p_sample_loop.one_step, at timestep t, noise injected
        eng = unet.engine()
        ws = eng.workspace(B, 2 * B, 64, 64)
        stream = L.current_stream()
        eng.set_text(ws, emb.to(dev), mask.to(dev), torch.cat((torch.ones(B, dtype=torch.bool), torch.zeros(B, dtype=torch.bool))))
        sstate = im._stage_state(ws, sched, (B, 3, 64, 64), StageCall(0, T))
        ws.x.copy_(x)
        noise_dev = torch.zeros(T, B, 3, 64, 64, device=dev)
        noise_dev[T - 1 - t] = noise.to(dev)                       # mi_posterior_fwd reads the draw of step index T-1-t
        L.check(lib.mi_step_set(L.ptr(sstate.t_state), L.ptr(ws.times), B, t, stream), "mi_step_set")
        eng.prepare_step_tables(ws, T, sstate.t_state, stream)
        k_lo, k_hi, w = quantile_rank(n, 0.9)
        cp = L.MiCfgX0Params(B, n, L.ptr(ws.pred), 1, 3.0, L.ptr(ws.x), L.ptr(sstate.coef), L.ptr(sstate.t_state), 0, L.ptr(sstate.x0), L.ptr(sstate.hist))
        qp = L.MiQuantileParams(B, n, L.ptr(sstate.x0), k_lo, k_hi, w, L.ptr(sstate.hist), L.ptr(sstate.s_q), L.ptr(sstate.v_q), 1, 1)
        pp = L.MiPosteriorParams(B, n, T, L.ptr(sstate.x0), L.ptr(sstate.s_q), L.ptr(ws.x), L.ptr(sstate.coef), L.ptr(sstate.t_state),
                                 L.ptr(noise_dev), 0, 0, 0, 0)
        eng.run_step(ws, stream)
        L.check(lib.mi_cfg_x0_fwd(C.byref(cp), stream), "mi_cfg_x0_fwd")
        L.check(lib.mi_quantile_fwd(C.byref(qp), stream), "mi_quantile_fwd")
        L.check(lib.mi_posterior_fwd(C.byref(pp), stream), "mi_posterior_fwd")
        torch.cuda.synchronize()
        assert (ws.x.cpu() - st["x_prev"]).abs().max() < 1e-4
        # the selected threshold is the reference's, bit for bit, given the same x0
        x0 = sstate.x0.cpu().reshape(B, -1)
        assert torch.equal(sstate.s_q.cpu(), torch.quantile(x0.abs(), 0.9, dim=-1).clamp(min=1.))
        # and the oracle's step on the kernels' own prediction agrees with the reference too
        xp, aux = R.p_sample(None, R.Schedule(T), x, t, noise, pred=pred.cpu())
        assert (xp - st["x_prev"]).abs().max() < 1e-4


@pytest.mark.parametrize("backend", BACKENDS)
def test_determinism_graph_and_sharding(backend):
    dev = setup(backend)
    gpu = backend == "gpu"
    T, B, cs = (25, 4, 3.) if gpu else (21, 2, 1.)                     # the emulator runs the same launches ~1e4x slower: fewer rows, no CFG,
    im = make_imagen([64 if gpu else 32], T, dev)                      # ... and a 32 x 32 image
    emb, mask = R.synthetic_text(B, length=16, seed=7)
    emb, mask = emb.to(dev), mask.to(dev)
    a = im.sample(text_embeds=emb, text_masks=mask, cond_scale=cs, _seed=11)
    c = im.sample(text_embeds=emb, text_masks=mask, cond_scale=cs, _seed=11, _use_graph=False)
    assert torch.equal(a, c)                                           # HIP-graph replay == eager launches, run-to-run bit-identical
    if gpu:
        b = im.sample(text_embeds=emb, text_masks=mask, cond_scale=cs, _seed=11)
        assert torch.equal(a, b)                                       # second call replays the cached graph
        d = im.sample(text_embeds=emb, text_masks=mask, cond_scale=cs, _seed=12)
        assert not torch.equal(a, d)                                   # ... and the device-side seed is live in it
        b = im.sample(text_embeds=emb, text_masks=mask, cond_scale=cs, _seed=11)
        assert torch.equal(a, b)
    h = B // 2                                                         # rank 1 of 2 sampling rows [h, B)
    e = im.sample(text_embeds=emb[h:].contiguous(), text_masks=mask[h:].contiguous(), cond_scale=cs, _seed=11, _sample_offset=h)
    assert torch.equal(e, a[h:])                                       # sharded rows == unsharded rows, bit for bit
    assert a.min() >= 0. and a.max() <= 1.


@pytest.mark.parametrize("backend", GPU_ONLY)
def test_cascade_full_size_vs_oracle(backend):
    """BASELINE sizes (base 64 -> SR 256, cond_scale 3, T = 25 per stage, B = 2): VALUES against the oracle on the same injected noise,
    max|d| <= 1e-4 and mean|d| <= 1e-5 on [0,1] images; then determinism / sharding invariance with on-device noise at B = 4"""
    dev = setup(backend)
    im = make_imagen([64, 256], 25, dev)
    emb, mask = R.synthetic_text(2, length=48, seed=9)
    out = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., _noise=R.make_randn(21))
    ref = R.sample([I.load("unet0_sd.pt"), I.load("unet1_sd.pt")], [64, 256], 25, text_embeds=emb, text_masks=mask, cond_scale=3., randn=R.make_randn(21))
    d = (out.cpu() - ref).abs()
    print(f"cascade 64->256 T=25 cs=3 B=2 vs oracle: max|d| = {d.max():.2e}, mean|d| = {d.mean():.2e}")
    assert out.shape == (2, 3, 256, 256) and d.max() < 1e-4 and d.mean() < 1e-5, (d.max(), d.mean())
    emb, mask = R.synthetic_text(4, length=64, seed=7)
    a = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., _seed=5)
    assert a.shape == (4, 3, 256, 256) and torch.isfinite(a).all() and a.min() >= 0 and a.max() <= 1
    e = im.sample(text_embeds=emb[2:].contiguous().to(dev), text_masks=mask[2:].contiguous().to(dev), cond_scale=3., _seed=5, _sample_offset=2)
    assert torch.equal(e, a[2:])


@pytest.mark.parametrize("backend", GPU_ONLY)
def test_three_stage_cascade_properties(backend):
    """BASELINE config 5 shape (64 -> 256 -> 1024, third U-Net = unet_1 params, noise augmentation on both SR stages), B=2:
    finite, in range, sharding-invariant"""
    dev = setup(backend)
    im = make_imagen([64, 256, 1024], 25, dev)
    emb, mask = R.synthetic_text(2, length=64, seed=7)
    a = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., lowres_sample_noise_level=0.2, _seed=5)
    assert a.shape == (2, 3, 1024, 1024) and torch.isfinite(a).all() and a.min() >= 0 and a.max() <= 1
    assert a.std() > 0.01
    e = im.sample(text_embeds=emb[1:].contiguous().to(dev), text_masks=mask[1:].contiguous().to(dev), cond_scale=3., _seed=5, _sample_offset=1)
    assert torch.equal(e, a[1:])
    # two calls in flight on the two call lanes: their 1024^2 stages overlap.  (Round 4: the grouped sampler tail with 128 workgroups per
    # image starved its own second launch there -- profiles/r04_sampler_group_config5.txt; the host keeps it to <= 8 workgroups per image.)
    # B = 4: 512 workgroups per launch at 128 per image, more than the chip holds at once (reproduces with MINIMAGEN_SAMPLER_GROUP_MAX=256)
    emb4, mask4 = R.synthetic_text(4, length=64, seed=7)
    kw = dict(text_embeds=emb4.to(dev), text_masks=mask4.to(dev), cond_scale=3., lowres_sample_noise_level=0.2)
    a = im.sample(**kw, _seed=5).clone()
    torch.cuda.synchronize()
    x = im.sample(**kw, _seed=5, _async=True)
    y = im.sample(**kw, _seed=5, _async=True)
    torch.cuda.synchronize()
    assert torch.equal(x, a) and torch.equal(y, a)
    im.check_device_status()
    from minimagen_amd import Imagen as IM
    st = [v for u in im.unets for ws in u.engine()._ws.values() for v in ws.__dict__.get("sampler_state", {}).values()]
    assert [hasattr(v, "group_sync") for v in st].count(True) >= 1          # the 256^2 stage took the grouped kernel ...
    assert IM.SAMPLER_GROUP_MAX == 8 and L.lib().mi_sampler_group_size(3 * 1024 * 1024) == 128      # ... the 1024^2 stage must not


@pytest.mark.parametrize("backend", GPU_ONLY)
def test_async_pipelined_calls_equal_synchronous_calls(backend):
    """What bench.py times: back-to-back sample(_async=True) calls, each with DIFFERENT, FRESHLY ALLOCATED text embeddings and its own
    seed, the caller dropping its inputs as soon as sample() returns and immediately reusing the memory (the caching allocator hands
    the freed block to the next same-sized allocation on the caller's stream).  Every output must be bit-identical to the same call
    made synchronously, one at a time."""
    dev = setup(backend)
    im = make_imagen([64, 256], 50, dev)
    B, Ltxt, n_calls = 16, 64, 4          # large enough that the two stages really overlap for most of a call
    host = [R.synthetic_text(B, length=Ltxt, seed=30 + k) for k in range(n_calls)]
    sync = []
    for k, (emb, mask) in enumerate(host):
        sync.append(im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., _seed=100 + k).clone())
    torch.cuda.synchronize()
    outs, events = [], []
    for k, (emb, mask) in enumerate(host):
        e, m = emb.to(dev), mask.to(dev)
        outs.append(im.sample(text_embeds=e, text_masks=m, cond_scale=3., _seed=100 + k, _async=True))
        events.append(im.last_sample_done)
        del e, m
        # same-sized scratch allocations on the caller's stream, scribbled over at once: with the inputs' blocks back in the allocator's
        # pool this would overwrite embeddings a stage stream has not consumed yet
        junk_e = torch.full((B, Ltxt, 512), float('nan'), device=dev)
        junk_m = torch.zeros(B, Ltxt, dtype=torch.bool, device=dev)
        del junk_e, junk_m
    for ev in events:
        ev.synchronize()
    torch.cuda.synchronize()
    for k in range(n_calls):
        assert torch.equal(outs[k], sync[k]), f"pipelined call {k} differs from the synchronous one"
    assert not torch.equal(sync[0], sync[1])
    # and return_pil_images on the pipelined path waits for the last stage before the device -> host copy
    pil = im.sample(text_embeds=host[0][0].to(dev), text_masks=host[0][1].to(dev), cond_scale=3., _seed=100, _async=True, return_pil_images=True)
    import numpy as np
    want = sync[0].cpu().mul(255).to(torch.uint8).permute(0, 2, 3, 1).numpy()
    assert all(np.array_equal(np.asarray(pil[i]), want[i]) for i in range(B))


@pytest.mark.parametrize("backend", GPU_ONLY)
def test_kernels_of_two_streams_side_by_side_stay_bit_exact(backend):
    """The stage-pipelined sampler runs the base stage of call k+1 NEXT TO the super-resolution stage of call k.  Round 3 found the fused
    small-image sampler tail returning wrong pixels in that situation only (a compiler-generated packed-fp32 instruction with an SGPR
    operand misbehaves next to another kernel's matrix-core waves: profiles/r03_pk_f32_hazard.txt).  Here: (1) the tail kernel on fixed
    inputs under a CrossEmbed load on a second stream, (2) a whole base-stage U-Net evaluation under the SR U-Net's kernels -- both
    must reproduce their idle-GPU results bit for bit."""
    import ctypes as C
    from minimagen_amd import _lib as L
    from minimagen_amd.helpers import quantile_rank
    dev = setup(backend)
    lib = L.lib()
    im = make_imagen([64, 256], 100, dev)
    B, n, T = 16, 3 * 64 * 64, 100
    emb, mask = R.synthetic_text(B, length=32, seed=7)
    emb, mask = emb.to(dev), mask.to(dev)
    keep = torch.cat((torch.ones(B, dtype=torch.bool), torch.zeros(B, dtype=torch.bool)))
    engs, wss = [], []
    for stage, S in enumerate((64, 256)):
        eng = im.unets[stage].engine(); eng.pack()
        ws = eng.workspace(B, 2 * B, S, S)
        g = torch.Generator().manual_seed(stage)
        ws.x.copy_(torch.randn(ws.x.shape, generator=g)); ws.times.fill_(37)
        if ws.lowres is not None:
            ws.lowres.copy_(torch.randn(ws.lowres.shape, generator=g)); ws.lowres_times.fill_(20)
            eng.prepare_lowres(ws)
        eng.set_text(ws, emb, mask, keep)
        engs.append(eng); wss.append(ws)
    main, side = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    ce = [(fn, p_) for fn, p_, name in wss[1].prog if name == "crossembed"]

    def load(reps):
        with torch.cuda.stream(side):
            for _ in range(reps):
                for fn, p_ in ce:
                    fn(C.byref(p_), side.cuda_stream)

    # (1) the fused tail of a base-stage step
    g = torch.Generator().manual_seed(0)
    pred, x_in = torch.randn(2 * B, n, generator=g).to(dev), torch.randn(B, n, generator=g).to(dev)
    coef = im.noise_schedulers[0].sampler_coef_table().to(dev).contiguous()
    t_state = torch.full((1,), 37, dtype=torch.int32, device=dev)
    k_lo, k_hi, w = quantile_rank(n, 0.9)
    x = torch.empty_like(x_in)
    s_q, v_q = torch.zeros(B, device=dev), torch.zeros(B, 2, device=dev)
    seed_dev = torch.full((1,), 1234, dtype=torch.int64, device=dev)
    cp = L.MiCfgX0Params(B, n, L.ptr(pred), 1, 3.0, L.ptr(x), L.ptr(coef), L.ptr(t_state), 0, 0, 0)
    qp = L.MiQuantileParams(B, n, 0, k_lo, k_hi, w, 0, L.ptr(s_q), L.ptr(v_q), 1, 1)
    pp = L.MiPosteriorParams(B, n, T, 0, L.ptr(s_q), L.ptr(x), L.ptr(coef), L.ptr(t_state), 0, 1234, 0, 0, L.ptr(seed_dev))

    def tail():
        with torch.cuda.stream(main):
            x.copy_(x_in)
            L.check(lib.mi_sampler_step_small_fwd(C.byref(cp), C.byref(qp), C.byref(pp), main.cuda_stream), "small")
            return x.clone()
    torch.cuda.synchronize()
    ref = tail()
    torch.cuda.synchronize()
    wrong = 0
    for rep in range(4):
        load(150)
        outs = [tail() for _ in range(100)]
        torch.cuda.synchronize()
        wrong += sum(0 if torch.equal(o, ref) else 1 for o in outs)
    assert wrong == 0, f"{wrong} of 400 tail launches differ from the idle-GPU result"

    # (2) every kernel of the base-stage U-Net evaluation
    def outputs(ws):
        return [t for t in ws.tensors if t is not None and t.is_floating_point()] + [ws.pred]
    with torch.cuda.stream(main):
        engs[0].run(wss[0])
        ref0 = [t.clone() for t in outputs(wss[0])]
    torch.cuda.synchronize()
    for rep in range(6):
        with torch.cuda.stream(side):
            for _ in range(6):
                engs[1].run(wss[1])
        with torch.cuda.stream(main):
            got = []
            for _ in range(4):
                engs[0].run(wss[0])
                got.append([t.clone() for t in outputs(wss[0])])
        torch.cuda.synchronize()
        for gset in got:
            assert all(torch.equal(a, b) for a, b in zip(ref0, gset)), "base-stage U-Net evaluation differs under a concurrent SR load"

    # (3) the super-resolution U-Net evaluation as the VICTIM: under the base stage's kernels (one call lane's stage pipeline), and next to
    # a second SR evaluation on another stream (two call lanes: SR next to SR is the common case of the pipelined mode)
    ws1b = engs[1].workspace(B, 2 * B, 256, 256, lane=1)
    ws1b.x.copy_(wss[1].x); ws1b.times.copy_(wss[1].times)
    ws1b.lowres.copy_(wss[1].lowres); ws1b.lowres_times.copy_(wss[1].lowres_times)
    engs[1].prepare_lowres(ws1b)
    engs[1].set_text(ws1b, emb, mask, keep)
    torch.cuda.synchronize()
    with torch.cuda.stream(main):
        engs[1].run(wss[1])
        ref1 = [t.clone() for t in outputs(wss[1])]
    torch.cuda.synchronize()
    for aggressor in ("base", "sr"):
        for rep in range(4):
            with torch.cuda.stream(side):
                if aggressor == "base":
                    for _ in range(12):
                        engs[0].run(wss[0])
                else:
                    for _ in range(3):
                        engs[1].run(ws1b)
            with torch.cuda.stream(main):
                got = []
                for _ in range(2):
                    engs[1].run(wss[1])
                    got.append([t.clone() for t in outputs(wss[1])])
            torch.cuda.synchronize()
            for gset in got:
                assert all(torch.equal(a, b) for a, b in zip(ref1, gset)), f"SR U-Net evaluation differs next to a concurrent {aggressor}-stage evaluation"
        if aggressor == "sr":
            assert all(torch.equal(a, b) for a, b in zip(ref1, outputs(ws1b))), "the second lane's SR evaluation differs from the first lane's"


@pytest.mark.parametrize("backend", GPU_ONLY)
def test_three_stage_cascade_reduced_precision_values_vs_oracle(backend):
    """BASELINE config 5 names bf16: the three-stage cascade 64 -> 256 -> 1024 in the reduced-precision configuration (single fp16 term on
    the matrix cores, bf16 activation storage in all three U-Nets, noise augmentation on both SR stages) WITH VALUES against the fp32
    oracle: the half-precision gate of SURVEY.md 8(c), max|d| <= 3e-2 and mean|d| <= 3e-3 on [0,1] images"""
    dev = setup(backend)
    im = make_imagen([64, 256, 1024], 25, dev)
    emb, mask = R.synthetic_text(1, length=32, seed=13)
    out = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=1., lowres_sample_noise_level=0.2, _noise=R.make_randn(77),
                    _precision="half")
    for u, S in zip(im.unets, (64, 256, 1024)):
        ws = u.engine().workspace(1, 1, S, S, precision="half")
        assert ws.half and ws.store16, f"stage {S}: the reduced-precision plan fell back to fp32 storage"
    sd0, sd1 = I.load("unet0_sd.pt"), I.load("unet1_sd.pt")
    ref = R.sample([sd0, sd1, sd1], [64, 256, 1024], 25, text_embeds=emb, text_masks=mask, cond_scale=1., randn=R.make_randn(77),
                   lowres_sample_noise_level=0.2)
    d = (out.cpu() - ref).abs()
    print(f"cascade 64->256->1024 T=25 cs=1 B=1, reduced precision, vs the fp32 oracle: max|d| = {d.max():.2e}, mean|d| = {d.mean():.2e}")
    assert out.shape == (1, 3, 1024, 1024) and d.max() < 3e-2 and d.mean() < 3e-3, (d.max(), d.mean())


@pytest.mark.parametrize("backend", GPU_ONLY)
def test_three_stage_cascade_values_vs_oracle(backend):
    """BASELINE config 5's shape (64 -> 256 -> 1024, third U-Net = unet_1 params, noise augmentation on both SR stages) with VALUES:
    B=1, T=25, cond_scale 1, injected noise, against the oracle; max|d| <= 1e-4, mean|d| <= 1e-5 on [0,1] images"""
    dev = setup(backend)
    im = make_imagen([64, 256, 1024], 25, dev)
    emb, mask = R.synthetic_text(1, length=32, seed=13)
    out = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=1., lowres_sample_noise_level=0.2, _noise=R.make_randn(77))
    sd0, sd1 = I.load("unet0_sd.pt"), I.load("unet1_sd.pt")
    ref = R.sample([sd0, sd1, sd1], [64, 256, 1024], 25, text_embeds=emb, text_masks=mask, cond_scale=1., randn=R.make_randn(77),
                   lowres_sample_noise_level=0.2)
    d = (out.cpu() - ref).abs()
    print(f"cascade 64->256->1024 T=25 cs=1 B=1 vs oracle: max|d| = {d.max():.2e}, mean|d| = {d.mean():.2e}")
    assert out.shape == (1, 3, 1024, 1024) and d.max() < 1e-4 and d.mean() < 1e-5, (d.max(), d.mean())


@pytest.mark.parametrize("backend", GPU_ONLY)
@pytest.mark.parametrize("sizes,B", [([64], 2), ([64, 256], 2)])
def test_half_precision_uses_bf16_storage(backend, sizes, B):
    """the reduced-precision configuration of the BASELINE U-Nets must really store its activations as bf16 (engine.workspace falls back
    to fp32 storage silently when a layer has no bf16-reading kernel: that must not happen for unet_0 / unet_1)"""
    dev = setup(backend)
    im = make_imagen(sizes, 25, dev)
    emb, mask = R.synthetic_text(B, length=16, seed=7)
    im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., _seed=3, _precision="half")
    for unet, S in zip(im.unets, sizes):
        ws = unet.engine().workspace(B, 2 * B, S, S, precision="half")
        assert ws.half and ws.store16, f"stage {S}: fp32 storage fallback"
        acts = [t for t in ws.tensors if t is not None and t.dim() == 4 and t.shape[-1] == S]
        assert acts and all(t.dtype == torch.bfloat16 for t in acts if t is not ws.pred)
        assert ws.pred.dtype == torch.float32                                   # the prediction feeds the fp32 sampler
        ws32 = unet.engine().workspace(B, 2 * B, S, S, precision="fp32")
        assert not ws32.store16


_BASE = dict(dim=8, dim_mults=(1, 2), num_resnet_blocks=1, layer_attns=False, layer_cross_attns=False, memory_efficient=False)
_SR = dict(dim=8, dim_mults=(1, 2), num_resnet_blocks=(1, 2), layer_attns=False, layer_cross_attns=False, memory_efficient=True)
ARG_SWEEP = {   # Imagen kwargs, sample kwargs, image sizes, batch, caption length
    "percentile_095": (dict(dynamic_thresholding_percentile=0.95), dict(cond_scale=2.), [32], 3, 10),
    "lowres_noise_05": (dict(lowres_sample_noise_level=0.5), dict(cond_scale=1.), [32, 64], 2, 10),
    "no_text_mask": (dict(), dict(cond_scale=2., nomask=True), [32], 2, 10),
    "caption_longer_than_256": (dict(), dict(cond_scale=2.), [32], 2, 300),
    "one_channel": (dict(channels=1), dict(cond_scale=2.), [32], 2, 10),
    "odd_batch_no_guidance": (dict(), dict(cond_scale=1.), [32], 5, 10),
}


@pytest.mark.parametrize("backend", GPU_ONLY)
@pytest.mark.parametrize("case", sorted(ARG_SWEEP))
def test_sampler_argument_sweep_vs_oracle(backend, case):
    """Imagen / sample() arguments away from the BASELINE parameter files, full sample() against the oracle (same injected noise)"""
    dev = setup(backend)
    ikw, skw, sizes, B, Ltxt = ARG_SWEEP[case]
    skw = dict(skw)
    torch.manual_seed(2)
    ch = ikw.get("channels", 3)
    unets = [Unet(**{**_BASE, "channels": ch})] + [Unet(**{**_SR, "channels": ch, "lowres_cond": True}) for _ in sizes[1:]]
    im = Imagen(unets, text_encoder_name="t5_small", image_sizes=sizes, timesteps=25, cond_drop_prob=0.15, **ikw)
    sds = [{k: v.clone() for k, v in u.state_dict().items()} for u in im.unets]
    im = im.to(dev)
    emb, mask = R.synthetic_text(B, length=Ltxt, seed=3)
    if skw.pop("nomask", False):
        mask = None
    out = im.sample(text_embeds=emb.to(dev), text_masks=None if mask is None else mask.to(dev), _noise=R.make_randn(5), **skw)
    ref = R.sample(sds, sizes, 25, text_embeds=emb, text_masks=mask, cond_scale=skw.get("cond_scale", 1.), randn=R.make_randn(5),
                   lowres_sample_noise_level=ikw.get("lowres_sample_noise_level", 0.2), percentile=ikw.get("dynamic_thresholding_percentile", 0.9), channels=ch)
    d = (out.cpu() - ref).abs()
    assert d.max() < 1e-4 and d.mean() < 1e-5, (d.max(), d.mean())


@pytest.mark.parametrize("backend", BACKENDS)
def test_grouped_sampler_tail_in_the_sampling_loop(backend, monkeypatch):
    """images too large for the one-workgroup tail (n > 16384) take mi_sampler_step_group_fwd: same pixels as the separate kernels, bit
    for bit, through graphs of several steps (the step offsets), with injected noise and with the on-device generator; and the oracle's
    values.  (The emulator runs a smaller image -- one workgroup per image; tests/test_kernels.py covers 2 and 4 there.)"""
    from minimagen_amd import Imagen as IM
    dev = setup(backend)
    gpu = backend == "gpu"
    torch.manual_seed(4)
    S, T = (96, 25) if gpu else (76, 25)                       # n = 27648: two workgroups per image / 17328: one
    kw = dict(dim=8, dim_mults=(1, 2), num_resnet_blocks=1, layer_attns=False, layer_cross_attns=False, memory_efficient=True)
    sd = {k: v.clone() for k, v in Unet(**kw).state_dict().items()}
    emb, mask = R.synthetic_text(2, length=10, seed=3)
    outs = {}
    for grp in (1, 0):
        monkeypatch.setattr(IM, "SAMPLER_GROUP", grp)
        im = Imagen([Unet(**kw)], text_encoder_name="t5_small", image_sizes=[S], timesteps=T, cond_drop_prob=0.15)
        im.unets[0].load_state_dict(sd)
        im = im.to(dev)
        args = dict(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=2.)
        outs[grp, "gen"] = im.sample(**args, _seed=11).cpu()
        if gpu:
            outs[grp, "gen2"] = im.sample(**args, _seed=11).cpu()          # the cached graph again, on the same sync words
            outs[grp, "noise"] = im.sample(**args, _noise=R.make_randn(5)).cpu()
        im.check_device_status()
        st = next(iter(im.unets[0].engine()._ws.values())).sampler_state
        assert any(hasattr(v, "group_sync") for v in st.values()) == bool(grp)
    assert torch.equal(outs[1, "gen"], outs[0, "gen"])
    assert outs[1, "gen"].isfinite().all() and outs[1, "gen"].std() > 0.01
    if gpu:
        assert torch.equal(outs[1, "gen2"], outs[1, "gen"]) and torch.equal(outs[1, "noise"], outs[0, "noise"])
        ref = R.sample([sd], [S], T, text_embeds=emb, text_masks=mask, cond_scale=2., randn=R.make_randn(5))
        assert (outs[1, "noise"] - ref).abs().max() < 1e-4


@pytest.mark.parametrize("backend", BACKENDS)
def test_grouped_sampler_tail_failure_is_loud_and_self_healing(backend):
    """A cooperative launch that cannot complete must never hand back a plausible image.  Fault injection (sync header word 12, bit 31:
    workgroup 1 of image 0 skips one arrival) + a short spin limit (its low bits) make the grouped tail of the NEXT call time out:
      * the tensor-returning sample() of that call yields NaN images (fail-stop: every workgroup that sees the sticky word poisons its part),
      * the next API entry -- sample() itself, wait_pending_samples() or check_device_status() -- raises MinImagenHipError,
      * after the exception the stage has re-zeroed its sync words and runs the separate kernels: the following call is bit-identical to
        a healthy run."""
    dev = setup(backend)
    torch.manual_seed(4)
    S, T, B = (96, 25, 2) if backend == "gpu" else (76, 25, 1)      # n = 27648: two workgroups per image (the emulator: 17328, one)
    kw = dict(dim=8, dim_mults=(1, 2), num_resnet_blocks=1, layer_attns=False, layer_cross_attns=False, memory_efficient=True)
    im = Imagen([Unet(**kw)], text_encoder_name="t5_small", image_sizes=[S], timesteps=T, cond_drop_prob=0.15).to(dev)
    emb, mask = R.synthetic_text(B, length=10, seed=3)
    args = dict(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=2., _seed=11)
    good = im.sample(**args).clone()
    assert good.isfinite().all()
    st = next(v for ws in im.unets[0].engine()._ws.values() for v in ws.sampler_state.values() if hasattr(v, "group_sync"))
    assert L.lib().mi_sampler_group_size(3 * S * S) == (2 if backend == "gpu" else 1)
    knobs = torch.tensor([2000 - 2 ** 31], dtype=torch.int32).view(torch.uint8)    # spin limit 2000 | bit 31: fault injection
    st.group_sync[12:16] = knobs.to(st.group_sync.device)
    bad = im.sample(**args)                                   # returns (the check is deferred) ...
    if backend == "gpu":
        torch.cuda.synchronize()
    assert torch.isnan(bad).all(), "a failed cooperative launch must leave NaN, not a stale image"     # ... with a visibly invalid result
    with pytest.raises(L.MinImagenHipError, match="0x301"):
        im.sample(**args)                                     # ... and the next API entry raises, from the tensor-returning path
    assert st.group_failed
    healed = im.sample(**args)                                # sync words re-zeroed, separate kernels from here on
    assert torch.equal(healed, good)
    im.check_device_status()
    if backend != "gpu":
        return                                  # (emulator time)
    # the same through the explicit status poll
    im2 = Imagen([Unet(**kw)], text_encoder_name="t5_small", image_sizes=[S], timesteps=T, cond_drop_prob=0.15).to(dev)
    im2.sample(**args)
    st2 = next(v for ws in im2.unets[0].engine()._ws.values() for v in ws.sampler_state.values() if hasattr(v, "group_sync"))
    st2.group_sync[12:16] = knobs.to(st2.group_sync.device)
    im2.sample(**args)
    with pytest.raises(L.MinImagenHipError, match="timed out"):
        im2.check_device_status()
    im2.check_device_status()                                 # reported once; the stage has fallen back
    assert im2.sample(**args).isfinite().all()


@pytest.mark.parametrize("backend", BACKENDS)
def test_deferred_weight_validation_tokens(backend):
    """engine.pack_identity / pack_begin / pack_changed (what sample() uses): unchanged weights -> no change; a ``p.data`` update (no version bump)
    -> changed, and pack() re-packs; a REPLACED parameter object -> changed as well"""
    dev = setup(backend)
    torch.manual_seed(4)
    u = Unet(dim=8, dim_mults=(1, 2), num_resnet_blocks=1, layer_attns=False, layer_cross_attns=False, memory_efficient=True).to(dev).eval()
    eng = u.engine()
    eng.pack_identity()
    pk = eng._pack
    assert pk is not None and not eng.pack_changed(eng.pack_begin())
    with torch.no_grad():
        u.final_conv.weight.data.mul_(1.5)
    assert eng.pack_changed(eng.pack_begin())
    eng.pack()
    assert eng._pack is not pk and not eng.pack_changed(eng.pack_begin())
    u.final_conv.bias = torch.nn.Parameter(u.final_conv.bias.detach().clone())
    assert eng.pack_changed(eng.pack_begin())
    eng.pack()
    assert not eng.pack_changed(eng.pack_begin())


@pytest.mark.parametrize("backend", GPU_ONLY)
def test_sample_notices_weight_updates_made_through_data(backend):
    """sample() validates the packed weights with a DEFERRED content-fingerprint check (engine.pack_begin / pack_changed: the verdict is read
    after the call's work is enqueued).  A ``p.data`` update between two calls bumps no version counter; the second call must still return
    the images of the NEW weights (it discards what it enqueued on the stale packs and runs again)."""
    dev = setup(backend)
    torch.manual_seed(4)
    kw = dict(dim=8, dim_mults=(1, 2), num_resnet_blocks=1, layer_attns=False, layer_cross_attns=False, memory_efficient=True)
    S = 32 if backend == "gpu" else 16
    im = Imagen([Unet(**kw)], text_encoder_name="t5_small", image_sizes=[S], timesteps=25, cond_drop_prob=0.15).to(dev)
    emb, mask = R.synthetic_text(2, length=10, seed=3)
    args = dict(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=2., _seed=11)
    a = im.sample(**args).clone()
    with torch.no_grad():
        for name, prm in im.unets[0].named_parameters():
            if name.endswith("final_conv.weight") or "init_conv" in name:
                prm.data.mul_(1.25)                          # no version bump
    b = im.sample(**args).clone()
    assert not torch.equal(a, b)
    im2 = Imagen([Unet(**kw)], text_encoder_name="t5_small", image_sizes=[S], timesteps=25, cond_drop_prob=0.15)
    im2.unets[0].load_state_dict({k: v.detach().cpu() for k, v in im.unets[0].state_dict().items()})
    im2 = im2.to(dev)
    assert torch.equal(im2.sample(**args), b)
    assert torch.equal(im.sample(**args), b)                 # and the steady state stays on the new packs
    # the call that is issued again keeps its keywords: the same kind of update, followed by a call with non-default ones
    g = torch.Generator().manual_seed(6)
    more = dict(args, sample_steps=5, sampler="ddim", init_images=torch.rand(2, 3, S, S, generator=g).to(dev), init_strength=0.6)
    with torch.no_grad():
        for name, prm in im.unets[0].named_parameters():
            if name.endswith("final_conv.weight") or "init_conv" in name:
                prm.data.mul_(0.8)
    c = im.sample(**more).clone()
    im3 = Imagen([Unet(**kw)], text_encoder_name="t5_small", image_sizes=[S], timesteps=25, cond_drop_prob=0.15)
    im3.unets[0].load_state_dict({k: v.detach().cpu() for k, v in im.unets[0].state_dict().items()})
    assert torch.equal(im3.to(dev).sample(**more), c) and not torch.equal(im2.sample(**more), c)


@pytest.mark.parametrize("backend", BACKENDS)
def test_degenerate_T20_schedule_is_all_nan_like_the_reference(backend):
    """timesteps=20 passes the reference's assert (diffusion_model.py:24) but gives beta_T = 1: sqrt_recip_alphas_cumprod[T-1] is
    inf, x0 becomes inf - inf, torch.quantile / clamp propagate the NaN and the reference returns an all-NaN image.  Same here."""
    dev = setup(backend)
    torch.manual_seed(2)
    u = Unet(dim=8, dim_mults=(1, 2), num_resnet_blocks=1, layer_attns=False, layer_cross_attns=False, memory_efficient=True)
    im = Imagen([u], text_encoder_name="t5_small", image_sizes=[16], timesteps=20, cond_drop_prob=0.15)
    sd = {k: v.clone() for k, v in im.unets[0].state_dict().items()}
    im = im.to(dev)
    emb, mask = R.synthetic_text(2, length=10, seed=3)
    out = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=2., _noise=R.make_randn(5))
    ref = R.sample([sd], [16], 20, text_embeds=emb, text_masks=mask, cond_scale=2., randn=R.make_randn(5))
    assert torch.isnan(ref).all() and torch.isnan(out).all()


def test_api_errors():
    setup("emu")
    im = make_imagen([64], 25, "cpu", cond_drop_prob=0.)
    emb, mask = R.synthetic_text(1, length=8, seed=1)
    with pytest.raises(AssertionError):
        im.sample(text_embeds=emb, text_masks=mask, cond_scale=3.)      # Imagen.py:291-295: no CFG without cond dropout
    with pytest.raises(AssertionError):
        im.sample()                                                      # Imagen.py:454
    with pytest.raises(AssertionError):
        im.sample(text_embeds=torch.zeros(1, 4, 100))                    # Imagen.py:455-456
    with pytest.raises(TypeError):
        Imagen(Unet(**I.unet_params()["unet0"]), text_encoder_name="t5_small", image_sizes=64)     # Imagen.py:107 quirk: len(int)
    assert [k for k in im.state_dict().keys() if not k.startswith("unets.")] == []                 # Appendix B-9
