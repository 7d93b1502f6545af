"""Negative prompts and guidance rescale of Imagen.sample: argument validation and the ABI on the host, the two rescale
launches against fp64 and the text kernel's text_rows through the C ABI, the sampling loop against a restated loop, and the invariants of
the loop (tail forms, inpainting, graph reuse, the untouched default call)."""
import ctypes as C

import pytest
import torch

from minimagen_amd import _lib as L
from minimagen_amd.Imagen import Imagen
from minimagen_amd.Unet import Unet
from minimagen_amd.diffusion_model import GaussianDiffusion
from oracle import resize_restated
from oracle import restated as R
from tests import _inputs as I
from tests._backend import BACKENDS, GPU_ONLY, setup
from tests.test_sample_steps import TINY, gate, make_imagen, tiny_imagen

EMU_ONLY = [pytest.param("emu", marks=pytest.mark.emu)]


def _sync(backend):
    if backend == "gpu":
        torch.cuda.synchronize()


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ 1. host, no kernel
def test_argument_validation():
    """bad values raise ValueError before anything is launched (no backend is loaded here: a launch would need one)"""
    im = Imagen([Unet(**TINY)], text_encoder_name="t5_small", image_sizes=[16], timesteps=25, cond_drop_prob=0.15)
    emb, mask = R.synthetic_text(2, length=8, seed=1)
    neg, nmask = R.synthetic_text(2, length=8, seed=2)
    neg5, nmask5 = R.synthetic_text(2, length=5, seed=2)
    ok = dict(text_embeds=emb, text_masks=mask, cond_scale=3.)
    bad = [dict(ok, guidance_rescale=-0.1), dict(ok, guidance_rescale=1.5), dict(ok, guidance_rescale=True), dict(ok, guidance_rescale="0.5"),
           dict(ok, guidance_rescale=float("nan")),
           dict(ok, negative_text_embeds=neg[:1], negative_text_masks=nmask[:1]),                        # batch
           dict(ok, negative_texts=["a"]), dict(ok, negative_texts=["a", "b", "c"]), dict(ok, negative_texts=[1, 2]),
           dict(ok, negative_text_embeds=neg[:, :, :256], negative_text_masks=nmask),                      # embedding dimension
           dict(ok, negative_texts=["a", "b"], negative_text_embeds=neg, negative_text_masks=nmask),      # both
           dict(ok, negative_text_masks=nmask),                                                            # a mask without embeddings
           dict(ok, negative_text_embeds=neg, negative_text_masks=nmask[:, :5]),                           # mask shape
           dict(ok, negative_text_embeds=neg),                                                             # one side masked, the other not
           dict(text_embeds=emb, cond_scale=3., negative_text_embeds=neg, negative_text_masks=nmask),
           dict(text_embeds=emb, cond_scale=3., negative_texts=["a", "b"]),
           dict(text_embeds=emb, cond_scale=3., negative_text_embeds=neg5),                                # unmasked, different lengths
           dict(ok, negative_text_embeds=neg[0], negative_text_masks=nmask),                               # not [B, L, E]
           dict(text_embeds=emb, text_masks=mask, guidance_rescale=0.5),                                   # cond_scale == 1
           dict(text_embeds=emb, text_masks=mask, cond_scale=1., negative_text_embeds=neg, negative_text_masks=nmask),
           dict(text_embeds=emb, text_masks=mask, cond_scale=1., negative_texts="blurry")]
    for kw in bad:
        with pytest.raises(ValueError):
            im.sample(**kw)
    with pytest.raises(TypeError):
        im.sample(emb, None, None, 3., None, False, None, 0.5)           # keyword-only
    args = (2, 3., None, emb, mask)
    assert im._parse_guidance(*args, None, None, None, None) == (0., None) and im._parse_guidance(*args, None, None, None, 0) == (0., None)
    assert im._parse_guidance(*args, None, None, None, 1) == (1., None)
    assert im._parse_guidance(*args, "blurry", None, None, 0.25) == (0.25, ["blurry", "blurry"])
    phi, (e, m) = im._parse_guidance(*args, None, neg5, nmask5, None)              # masked on both sides: the lengths may differ
    assert phi == 0. and e.shape == neg5.shape and m.shape == nmask5.shape


def test_padding_rule_for_masked_inputs_of_different_lengths():
    """the shorter side gets zero embeddings under a False mask, on either side; without masks the lengths must agree"""
    from minimagen_amd.engine import join_negative
    emb, mask = R.synthetic_text(2, length=9, seed=1)
    neg, nmask = R.synthetic_text(2, length=5, seed=2)
    for (a, am), (b, bm) in (((emb, mask), (neg, nmask)), ((neg, nmask), (emb, mask))):
        e, m = join_negative(a, am, b, bm)
        assert e.shape == (4, 9, 512) and m.shape == (4, 9) and m.dtype == torch.bool
        for rows, (src, sm) in ((slice(0, 2), (a, am)), (slice(2, 4), (b, bm))):
            ln = src.shape[1]
            assert torch.equal(e[rows, :ln], src) and torch.equal(m[rows, :ln], sm)
            assert (e[rows, ln:] == 0).all() and not m[rows, ln:].any()
    e, m = join_negative(emb, None, emb.flip(0), None)
    assert m is None and torch.equal(e[:2], emb) and torch.equal(e[2:], emb.flip(0))
    for args in ((emb, None, neg, None), (emb, mask, neg, None), (emb, None, neg, nmask), (emb, mask, neg[:1], nmask[:1]),
                 (emb, mask, neg[:, :, :8], nmask), (emb, mask, neg, nmask[:, :3])):
        with pytest.raises(ValueError):
            join_negative(*args)


@pytest.mark.parametrize("backend", BACKENDS)
def test_abi_is_additive(backend):
    setup(backend)
    lib = L.lib()
    assert lib.mi_abi_version() == 12
    assert C.sizeof(L.MiTextCondParams) == lib.mi_struct_size(4) == 192 and L.MiTextCondParams.text_rows.offset == 28
    assert L.MiTextCondParams.max_len.offset == 24 and L.MiTextCondParams.text_embeds.offset == 32
    assert lib.mi_struct_size(33) == C.sizeof(L.MiCfgRescaleParams) == 32
    assert lib.mi_struct_size(30) == -1
    assert [lib.mi_cfg_rescale_chunks(n) for n in (0, 1, 4096, 4097, 12288, 196608)] == [0, 1, 1, 2, 3, 48]
    for name in ("mi_cfg_rescale_stats_fwd", "mi_cfg_rescale_apply_fwd"):
        getattr(lib, name)


def test_forwarding_entry_points_pass_the_keywords(tmp_path, monkeypatch):
    """generate.sample_and_save(sample_args=) and distributed.sample_distributed(**kwargs) hand the guidance keywords to Imagen.sample (a
    recording stand-in for the model: no backend needed), the negative tensors sharded by the captions' row bounds, and say so"""
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

    generate.sample_and_save(["a", "b"], minimagen=Recorder(), sample_args=dict(cond_scale=3., negative_texts="blurry", guidance_rescale=0.7),
                             save_directory=str(tmp_path / "out"))
    assert seen[-1]["negative_texts"] == "blurry" and seen[-1]["guidance_rescale"] == 0.7 and seen[-1]["cond_scale"] == 3.
    neg, nmask = torch.arange(3 * 4 * 16, dtype=torch.float32).reshape(3, 4, 16), torch.ones(3, 4, dtype=torch.bool)
    out = distributed.sample_distributed(Recorder(), text_embeds=torch.zeros(3, 4, 16), text_masks=torch.ones(3, 4, dtype=torch.bool), cond_scale=3.,
                                         negative_text_embeds=neg, negative_text_masks=nmask, guidance_rescale=0.5)
    assert out.shape[0] == 3 and seen[-1]["guidance_rescale"] == 0.5
    assert torch.equal(seen[-1]["negative_text_embeds"], neg) and torch.equal(seen[-1]["negative_text_masks"], nmask)       # one rank: every row
    # rank 1 of 2 (no process group: the three queries are stood in for, gather=False): rows shard_bounds(3, 2, 1) of every per-row tensor
    monkeypatch.setattr(distributed.dist, "is_initialized", lambda: True)
    monkeypatch.setattr(distributed.dist, "get_world_size", lambda group=None: 2)
    monkeypatch.setattr(distributed.dist, "get_rank", lambda group=None: 1)
    lo, hi = distributed.shard_bounds(3, 2, 1)
    assert (lo, hi) == (2, 3)
    out = distributed.sample_distributed(Recorder(), text_embeds=torch.zeros(3, 4, 16), text_masks=torch.ones(3, 4, dtype=torch.bool), cond_scale=3.,
                                         negative_text_embeds=neg, negative_text_masks=nmask, guidance_rescale=0.5, gather=False)
    assert out.shape[0] == 1 and seen[-1]["_sample_offset"] == lo and seen[-1]["text_embeds"].shape[0] == 1
    assert torch.equal(seen[-1]["negative_text_embeds"], neg[lo:hi]) and torch.equal(seen[-1]["negative_text_masks"], nmask[lo:hi])
    for fn in (generate.sample_and_save, distributed.sample_distributed):
        assert "negative_text_embeds" in fn.__doc__ and "guidance_rescale" in fn.__doc__


# ------------------------------------------------------------------------------------------------ 2. the rescale launches against fp64
def run_rescale(backend, dev, c, u, s, phi):
    """-> (pred2 after the two launches [2B, n], partials [B, chunks, 4]), on the host"""
    lib = L.lib()
    B, n = c.shape
    pred2 = torch.cat((c, u)).contiguous().to(dev)
    part = torch.zeros(B, lib.mi_cfg_rescale_chunks(n), 4, dtype=torch.float64, device=dev)
    p = L.MiCfgRescaleParams(B, n, pred2.data_ptr(), s, phi, part.data_ptr())
    L.check(lib.mi_cfg_rescale_stats_fwd(C.byref(p), L.current_stream()), "mi_cfg_rescale_stats_fwd")
    L.check(lib.mi_cfg_rescale_apply_fwd(C.byref(p), L.current_stream()), "mi_cfg_rescale_apply_fwd")
    _sync(backend)
    return pred2.cpu(), part.cpu()


def rescale_reference(c, u, s, phi):
    """g in fp32 torch ops (separate ops: the tails' three roundings), the standard deviations and f in fp64 from those fp32 values -> (g, g f in fp64)"""
    g = u + (c - u) * s
    sc, sg = c.double().std(dim=1, unbiased=False), g.double().std(dim=1, unbiased=False)
    f = torch.where(sg == 0, torch.ones_like(sg), phi * sc / sg + (1. - phi))
    return g, g.double() * f[:, None]


def check_rescale(out, c, u, s, phi, what):
    B = c.shape[0]
    g, ref = rescale_reference(c, u, s, phi)
    err = ((out[:B].double() - ref).abs() / ref.abs().clamp(min=1e-300)).max().item()
    print(f"{what}: max |out - ref| / |ref| = {err:.3e} = {err * 2 ** 24:.2f} x 2^-24 (gate 2^-22)")
    assert ((out[:B].double() - ref).abs() <= 2. ** -22 * ref.abs()).all(), (what, err)
    assert torch.equal(_bits(out[B:]), _bits(u)), what                    # the null / negative rows: untouched
    return g


RESCALE_CASES = [(1, 192, 3.0, 0.7), (2, 12288, 7.5, 1.0), (3, 4099, 0.5, 0.3), (2, 196608, 3.0, 0.5)]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("B,n,s,phi", RESCALE_CASES)
def test_rescale_kernels_vs_fp64(backend, B, n, s, phi):
    """less than one chunk | whole chunks (the base image) | odd n across a chunk boundary (no 16-byte accesses, a ragged last chunk) | many
    chunks (the SR image); plus the chunk sums themselves and, an image's result being a function of its own rows, another batch around it"""
    dev = setup(backend)
    gen = torch.Generator().manual_seed(100 + n % 97)
    c, u = torch.randn(B, n, generator=gen) * 0.8 + 0.1, torch.randn(B, n, generator=gen) * 0.7 - 0.05
    out, part = run_rescale(backend, dev, c, u, s, phi)
    g = check_rescale(out, c, u, s, phi, f"B={B} n={n} s={s} phi={phi}")
    for k, v in enumerate((c.double(), c.double() ** 2, g.double(), g.double() ** 2)):
        want = torch.stack([chunk.sum(dim=1) for chunk in v.split(4096, dim=1)], dim=1)
        assert ((part[:, :, k] - want).abs() <= 1e-12 * v.abs().sum(dim=1, keepdim=True)).all(), k
    last, _ = run_rescale(backend, dev, c[B - 1:], u[B - 1:], s, phi)
    assert torch.equal(_bits(last[:1]), _bits(out[B - 1:B]))


@pytest.mark.parametrize("backend", BACKENDS)
def test_rescale_hostile_rows(backend):
    """c and u = 100 + 0.01 randn: the variance is 1e-8 of the second moment -- why the sums are fp64"""
    dev = setup(backend)
    B, n, s, phi = 2, 12288, 7.5, 1.0
    gen = torch.Generator().manual_seed(5)
    c, u = 100 + 0.01 * torch.randn(B, n, generator=gen), 100 + 0.01 * torch.randn(B, n, generator=gen)
    out, _ = run_rescale(backend, dev, c, u, s, phi)
    check_rescale(out, c, u, s, phi, "hostile rows")


@pytest.mark.parametrize("backend", BACKENDS)
def test_rescale_constant_guided_prediction(backend):
    """sigma(g) == 0: f = 1 and the output is g to the bit (values whose sums and squares are exact in fp64)"""
    dev = setup(backend)
    for n in (192, 12288, 4099):
        gen = torch.Generator().manual_seed(n)
        c = torch.stack((torch.full((n,), 2.), torch.full((n,), 0.75), torch.randn(n, generator=gen)))
        u = torch.stack((torch.full((n,), 1.), torch.full((n,), 0.75), torch.randn(n, generator=gen)))
        out, _ = run_rescale(backend, dev, c, u, 3.0, 0.7)
        g = check_rescale(out, c, u, 3.0, 0.7, f"constant g, n={n}")
        assert torch.equal(_bits(out[:2]), _bits(g[:2])) and (out[0] == 4.).all() and (out[1] == 0.75).all()


@pytest.mark.parametrize("backend", BACKENDS)
def test_rescale_nan_is_fail_stop(backend):
    """one NaN element, in either half, makes its image's row NaN and leaves the other images' bits alone"""
    dev = setup(backend)
    B, n, s, phi = 3, 4099, 0.5, 0.3
    gen = torch.Generator().manual_seed(9)
    c, u = torch.randn(B, n, generator=gen), torch.randn(B, n, generator=gen)
    clean, _ = run_rescale(backend, dev, c, u, s, phi)
    for half, row, col in (("c", 1, 4097), ("u", 0, 17), ("c", 2, 0)):
        c2, u2 = c.clone(), u.clone()
        (c2 if half == "c" else u2)[row, col] = float("nan")
        out, _ = run_rescale(backend, dev, c2, u2, s, phi)
        assert out[row].isnan().all(), (half, row, col)
        others = [b for b in range(B) if b != row]
        assert torch.equal(_bits(out[others]), _bits(clean[others]))
        assert torch.equal(_bits(out[B:]), _bits(u2))


@pytest.mark.parametrize("backend", BACKENDS)
def test_rescale_rejects_bad_arguments(backend):
    dev = setup(backend)
    lib = L.lib()
    pred2, part = torch.zeros(2, 64, device=dev), torch.zeros(1, 1, 4, dtype=torch.float64, device=dev)
    good = (1, 64, pred2.data_ptr(), 3.0, 0.5, part.data_ptr())
    for k, v in ((0, 0), (1, 0), (1, -4), (2, 0), (3, float("inf")), (3, float("nan")), (4, 1.5), (4, -0.5), (4, float("nan")), (5, 0), (0, 70000)):
        args = list(good)
        args[k] = v
        p = L.MiCfgRescaleParams(*args)
        for fn in (lib.mi_cfg_rescale_stats_fwd, lib.mi_cfg_rescale_apply_fwd):
            assert fn(C.byref(p), L.current_stream()) == -1, (k, v)
    _sync(backend)
    assert (pred2 == 0).all()


# ------------------------------------------------------------------------------------------------ 3. the text kernel's text_rows
def _text_params(u, B2, B, emb, mask8, keep8, c_text, hid, text_rows):
    from minimagen_amd.engine import MAX_TEXT_LEN, _lin
    p = L.MiTextCondParams()
    p.B2, p.B, p.L, p.E, p.cd, p.tcd, p.max_len = B2, B, emb.shape[1], u.text_embed_dim, u.cond_dim, u.time_cond_dim, MAX_TEXT_LEN
    p.text_rows = text_rows
    p.text_embeds, p.text_mask, p.keep = L.ptr(emb), L.ptr(mask8), L.ptr(keep8)
    p.text_to_cond, p.null_text_embed = _lin(u.text_to_cond), L.ptr(u.null_text_embed)
    ln = u.to_text_non_attn_cond[0]
    p.ln_w, p.ln_b = L.ptr(ln.weight), L.ptr(ln.bias)
    p.h1, p.h2 = _lin(u.to_text_non_attn_cond[1]), _lin(u.to_text_non_attn_cond[3])
    p.null_text_hidden = L.ptr(u.null_text_hidden)
    p.norm_w, p.norm_b = L.ptr(u.norm_cond.weight), L.ptr(u.norm_cond.bias)
    p.c_text, p.text_hiddens = L.ptr(c_text), L.ptr(hid)
    return p


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("length", [5, 9])
def test_text_rows_per_guidance_row(backend, masked, length):
    """text_rows = B2: rows [B, 2B) are what the entry gives for the negative captions alone (a B-row call with keep = 1), rows [0, B) what it
    gives today -- bit for bit -- and both are the oracle's text conditioning of the concatenated batch (the golden base U-Net's cond_dim and
    time_cond_dim, E = 512)"""
    from minimagen_amd.engine import MAX_TEXT_LEN
    dev = setup(backend)
    p0 = I.unet_params()["unet0"]
    u, sd = Unet(**p0), I.load("unet0_sd.pt")
    u.load_state_dict(sd)
    u = u.to(dev)
    B, lib = 2, L.lib()
    emb, mask = R.synthetic_text(B, length=length, seed=5)
    neg, nmask = R.synthetic_text(B, length=length, seed=6)
    if masked:
        mask[1, 3:] = False
        nmask[0, 2:] = False
    else:
        mask = nmask = None
    both, both_mask = torch.cat((emb, neg)), (torch.cat((mask, nmask)) if masked else None)
    to8 = lambda m: None if m is None else m.to(torch.uint8).contiguous().to(dev)

    def run(B2, Bp, e, m, keep, text_rows):
        c_text, hid = torch.zeros(B2, MAX_TEXT_LEN, u.cond_dim, device=dev), torch.zeros(B2, u.time_cond_dim, device=dev)
        keep = (e.contiguous().to(dev), to8(m), keep.to(torch.uint8).to(dev))
        rc = lib.mi_text_cond_fwd(C.byref(_text_params(u, B2, Bp, *keep, c_text, hid, text_rows)), L.current_stream())
        _sync(backend)
        return rc, c_text.cpu(), hid.cpu()

    ones = torch.ones(2 * B)
    rc, c_all, h_all = run(2 * B, B, both, both_mask, ones, 2 * B)
    assert rc == 0
    for rows in (0, B):                                                      # 0 and B mean "text row bb % B", as before the field existed
        rc, c_neg, h_neg = run(B, B, neg, nmask, ones[:B], rows)
        assert rc == 0 and torch.equal(_bits(c_neg), _bits(c_all[B:])) and torch.equal(_bits(h_neg), _bits(h_all[B:]))
    rc, c_old, h_old = run(2 * B, B, emb, mask, torch.cat((ones[:B], torch.zeros(B))), 0)
    assert rc == 0 and torch.equal(_bits(c_old[:B]), _bits(c_all[:B])) and torch.equal(_bits(h_old[:B]), _bits(h_all[:B]))
    assert not torch.equal(c_old[B:], c_all[B:])                             # (the null rows are not the negative rows)
    for rows in (1, 3, -1, 8):
        assert run(2 * B, B, both, both_mask, ones, rows)[0] == -1
    t0, tok = R.generate_t_tokens(sd, torch.tensor([7, 3, 7, 3]), None)
    t1, c_ref = R.text_condition(sd, both, both_mask, torch.ones(2 * B, dtype=torch.bool), t0, tok)
    ntot = tok.shape[1]
    d_c, d_h = (c_all - c_ref[:, ntot:]).abs().max().item(), (h_all - (t1 - t0)).abs().max().item()
    print(f"text_rows = B2, L = {length}, masked = {masked}: max|d| c_text {d_c:.2e}, text hiddens {d_h:.2e}")
    assert d_c < 2e-5 and d_h < 2e-5


@pytest.mark.parametrize("backend", BACKENDS)
def test_set_text_joins_the_negative_rows(backend):
    """engine.set_text with negatives: ONE launch with text_rows = B2 over the joined captions, keep = 1 everywhere -- and back to the null rows
    on the next call without them (the keep pattern follows)"""
    dev = setup(backend)
    im, _ = tiny_imagen(16, 21, dev)
    eng = im.unets[0].engine()
    B = 2
    emb, mask = R.synthetic_text(B, length=9, seed=5)
    neg, nmask = R.synthetic_text(B, length=5, seed=6)
    ws = eng.workspace(B, 2 * B, 16, 16)
    keep = torch.cat((torch.ones(B, dtype=torch.bool), torch.zeros(B, dtype=torch.bool)))
    eng.set_text(ws, emb.to(dev), mask.to(dev), keep)
    _sync(backend)
    plain = ws.c_text.cpu().clone()
    eng.set_text(ws, emb.to(dev), mask.to(dev), keep, negative_embeds=neg.to(dev), negative_mask=nmask.to(dev))
    _sync(backend)
    with_neg = ws.c_text.cpu().clone()
    assert (ws.keep.cpu() == 1).all() and torch.equal(with_neg[:B], plain[:B]) and not torch.equal(with_neg[B:], plain[B:])
    ws2 = eng.workspace(B, 2 * B, 16, 16, lane=1)
    eng.set_text(ws2, neg.to(dev), nmask.to(dev), torch.ones(2 * B, dtype=torch.bool))          # the negative captions as captions
    _sync(backend)
    assert torch.equal(ws2.c_text.cpu()[:B], with_neg[B:])
    eng.set_text(ws, emb.to(dev), mask.to(dev), keep)
    _sync(backend)
    assert torch.equal(ws.c_text.cpu(), plain) and torch.equal(ws.keep.cpu(), keep.to(torch.uint8))


# ------------------------------------------------------------------------------------------------ 4. the sampling loop against a restated loop
def restated_guided_sample(sds, sizes, T, steps, sampler, eta, *, text_embeds, text_masks, cond_scale, randn, negative=None, phi=0.,
                           lowres_sample_noise_level=0.2):
    """tests.test_sample_steps.restated_sample with the guided prediction formed here: two R.unet_forward calls -- the captions, and the
    negative captions (``negative`` = (embeds, masks)) or cond_drop_prob = 1 -- combined as neg + (pos - neg) * cond_scale and, for phi > 0,
    scaled per image by phi * std(pos) / std(guided) + 1 - phi with the standard deviations in fp64"""
    b = text_embeds.shape[0]
    steps = (steps,) * len(sds) if isinstance(steps, int) else steps
    lowres_sched = R.Schedule(T)
    img = None
    for sd, size, S in zip(sds, sizes, steps):
        kw = {}
        if "to_lowres_time_hiddens.1.weight" in sd:
            lt = lowres_sched.get_times(b, lowres_sample_noise_level)
            low = resize_restated.resize(img, scale_factors=size / img.shape[-1], pad_mode='reflect') if img.shape[-1] != size else img
            low = lowres_sched.q_sample(low, int(lt[0]), randn(low.shape))
            kw.update(lowres_cond_img=low * 2 - 1, lowres_noise_times=lt)
        tau, tab = GaussianDiffusion(timesteps=T).sampler_tables(S, sampler, eta)
        shape = (b, 3, size, size)
        x, prev = randn(shape), torch.zeros(shape)
        for k in range(S - 1, -1, -1):
            t = torch.full((b,), int(tau[k]), dtype=torch.long)
            pos = R.unet_forward(sd, x, t, text_embeds=text_embeds, text_mask=text_masks, cond_drop_prob=0., **kw)
            if negative is None:
                neg = R.unet_forward(sd, x, t, text_embeds=text_embeds, text_mask=text_masks, cond_drop_prob=1., **kw)
            else:
                neg = R.unet_forward(sd, x, t, text_embeds=negative[0], text_mask=negative[1], cond_drop_prob=0., **kw)
            pred = neg + (pos - neg) * cond_scale
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


CASES = [pytest.param(0.7, False, id="rescale"), pytest.param(0., True, id="negatives"), pytest.param(0.7, True, id="both")]


def _captions(length, neg_length):
    """captions and (shorter: the padding rule is live) negative captions of B = 2, both masked"""
    emb, mask = R.synthetic_text(2, length=length, seed=9)
    neg, nmask = R.synthetic_text(2, length=neg_length, seed=10)
    nmask[1, neg_length // 2:] = False
    return emb, mask, neg.masked_fill(~nmask[:, :, None], 0.), nmask


def _sample_and_reference(im, sds, sizes, T, steps, sampler, dev, phi, negatives, length=48, neg_length=20, noise=21):
    emb, mask, neg, nmask = _captions(length, neg_length)
    kw = {} if not phi else dict(guidance_rescale=phi)
    if negatives:
        kw.update(negative_text_embeds=neg.to(dev), negative_text_masks=nmask.to(dev))
    out = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., _noise=R.make_randn(noise), sample_steps=steps, sampler=sampler, **kw)
    ref = restated_guided_sample(sds, sizes, T, steps, sampler, None, text_embeds=emb, text_masks=mask, cond_scale=3., randn=R.make_randn(noise),
                                 negative=(neg, nmask) if negatives else None, phi=phi)
    im.check_device_status()
    return out, ref


@pytest.mark.parametrize("backend", EMU_ONLY)
@pytest.mark.parametrize("phi,negatives", CASES)
def test_values_emulator(backend, phi, negatives):
    """tiny U-Net at 16^2, T = 21, 4 steps, B = 2, cond_scale 3.  (T = 21, not 20: the linear schedule's last beta is 0.02 * 1000 / T, which is
    exactly 1 at T = 20 -- abar_T = 0, infinite x0 coefficients at the first step, and every sample() of ANY kind, the restated loop
    included, is NaN there; 21 is the smallest T the emulator tests of tests/test_sample_steps.py use.)"""
    dev = setup(backend)
    im, sd = tiny_imagen(16, 21, dev)
    out, ref = _sample_and_reference(im, [sd], [16], 21, 4, "ddpm", dev, phi, negatives, length=12, neg_length=7)
    gate(out, ref, f"emulator 16^2 T=21 S=4 phi={phi} negatives={negatives}")


@pytest.mark.parametrize("backend", GPU_ONLY)
@pytest.mark.parametrize("sampler", ["ddpm", "dpmpp_2m"])
@pytest.mark.parametrize("phi,negatives", CASES)
def test_values_base_stage(backend, sampler, phi, negatives):
    """the golden base U-Net at 64^2, T = 25, 5 steps, B = 2, cond_scale 3"""
    dev = setup(backend)
    im = make_imagen([64], 25, dev)
    out, ref = _sample_and_reference(im, [I.load("unet0_sd.pt")], [64], 25, 5, sampler, dev, phi, negatives)
    gate(out, ref, f"base 64^2 T=25 S=5 {sampler} phi={phi} negatives={negatives}")


@pytest.mark.parametrize("backend", GPU_ONLY)
@pytest.mark.parametrize("phi", [0.7, 0.])
def test_values_cascade(backend, phi):
    """64 -> 256, T = 25, 5 steps per stage, B = 2, negatives: with phi = 0.7 the SR stage runs on the UNFOLDED workspace and the grouped tail
    reads B rescaled rows; with negatives alone it stays on the FOLDED workspace (the fold is linear in the two halves whatever text they saw)"""
    dev = setup(backend)
    im = make_imagen([64, 256], 25, dev)
    out, ref = _sample_and_reference(im, [I.load("unet0_sd.pt"), I.load("unet1_sd.pt")], [64, 256], 25, (5, 5), "ddpm", dev, phi, True)
    gate(out, ref, f"cascade 64->256 T=25 S=(5, 5) phi={phi} negatives")
    (key, ws), = im.unets[1].engine()._ws.items()
    if phi:
        assert key[-1] == "nofold" and ws.cfg_fold is None
    else:
        assert "nofold" not in key and ws.cfg_fold is not None
    (st,) = ws.sampler_state.values()
    assert hasattr(st, "group_sync") and (st.rescale_partials is not None) == bool(phi)


# ------------------------------------------------------------------------------------------------ 5. tail forms, inpainting, graphs
@pytest.mark.parametrize("backend", GPU_ONLY)
def test_three_tail_forms_agree_in_the_sampling_loop(backend, monkeypatch):
    """phi > 0 through the one-workgroup tail, the grouped tail and the separate kernels: identical bits"""
    from minimagen_amd import Imagen as IM
    dev = setup(backend)
    emb, mask = R.synthetic_text(2, length=10, seed=3)
    for S_img, kinds in ((24, ("small", "separate")), (96, ("group", "separate"))):
        outs = {}
        for kind in kinds:
            monkeypatch.setenv("MINIMAGEN_SAMPLER_FUSED", "0" if (kind == "separate" and S_img == 24) else "1")
            monkeypatch.setattr(IM, "SAMPLER_GROUP", 0 if kind == "separate" else 1)
            im, _ = tiny_imagen(S_img, 25, dev)
            outs[kind] = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=2., _seed=11, sample_steps=10, sampler="dpmpp_2m",
                                   guidance_rescale=0.7).cpu()
            im.check_device_status()
            (key, ws), = im.unets[0].engine()._ws.items()
            assert key[-1] == "nofold" and list(ws.sampler_state.keys()) == [(25, 10, "dpmpp_2m", 0.)]
            assert any(hasattr(v, "group_sync") for v in ws.sampler_state.values()) == (kind == "group")
        a, b = (outs[k] for k in kinds)
        assert torch.equal(a, b), kinds
        assert a.isfinite().all() and a.std() > 0.01


@pytest.mark.parametrize("backend", GPU_ONLY)
def test_inpainting_with_rescale_returns_the_known_pixels(backend):
    """a full mask with phi > 0 and negatives: the known image comes back within the three roundings of tests/test_inpaint.py (2^-22)"""
    dev = setup(backend)
    im = make_imagen([64], 25, dev)
    emb, mask, neg, nmask = _captions(16, 9)
    y = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(3))
    out = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., _seed=11, inpaint_images=y.to(dev),
                    inpaint_masks=torch.ones(2, 1, 64, 64, device=dev), guidance_rescale=0.7, negative_text_embeds=neg.to(dev),
                    negative_text_masks=nmask.to(dev)).cpu()
    d = (out - y).abs().max().item()
    print(f"full mask with phi = 0.7: max|d| = {d:.3e}")
    assert d <= 2. ** -22
    half = torch.zeros(2, 64, 64, dtype=torch.bool)
    half[:, :, :32] = True
    out = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., _seed=11, inpaint_images=y.to(dev), inpaint_masks=half.to(dev),
                    guidance_rescale=0.7).cpu()
    m = half[:, None].expand_as(out)
    assert (out - y)[m].abs().max() <= 2. ** -22 and out.isfinite().all() and (out - y)[~m].abs().max() > 0.05
    im.check_device_status()


@pytest.mark.parametrize("backend", GPU_ONLY)
def test_graph_reuse_and_sharding(backend):
    """other negative captions replay the captured graph and give another image; phi 0.7 -> 0.3 -> 0.7 gives the first image again (one graph
    per phi); graph == eager; sharded rows == unsharded rows with negatives and phi (the statistics are per image)"""
    dev = setup(backend)
    gpu = backend == "gpu"
    im = make_imagen([64], 25, dev) if gpu else tiny_imagen(16, 21, dev)[0]
    B = 4 if gpu else 2
    emb, mask = R.synthetic_text(B, length=16, seed=7)
    neg, nmask = R.synthetic_text(B, length=9, seed=8)
    neg2, nmask2 = R.synthetic_text(B, length=12, seed=12)
    emb, mask, neg, nmask, neg2, nmask2 = (t.to(dev) for t in (emb, mask, neg, nmask, neg2, nmask2))
    kw = dict(text_embeds=emb, text_masks=mask, cond_scale=3., _seed=11)
    states = lambda: [st for ws in im.unets[0].engine()._ws.values() for st in ws.sampler_state.values()]
    plain = im.sample(**kw).clone()
    a = im.sample(**kw, negative_text_embeds=neg, negative_text_masks=nmask).clone()
    (st,) = states()
    n_graphs = len(st.graphs)
    b = im.sample(**kw, negative_text_embeds=neg2, negative_text_masks=nmask2).clone()
    assert len(states()) == 1 and len(st.graphs) == n_graphs == 1                 # negatives change no key: the plain call's graph
    assert not torch.equal(a, b) and not torch.equal(a, plain) and a.isfinite().all() and b.isfinite().all()
    assert torch.equal(im.sample(**kw), plain)                                      # ... and back to the null rows
    r7 = im.sample(**kw, guidance_rescale=0.7).clone()
    r3 = im.sample(**kw, guidance_rescale=0.3).clone()
    assert torch.equal(im.sample(**kw, guidance_rescale=0.7), r7) and not torch.equal(r3, r7) and not torch.equal(r7, plain)
    assert r7.isfinite().all() and r7.std() > 0.01
    (_, st_r) = states()
    assert len(st_r.graphs) == 2 and all(k[-1][0] == "rescale" for k in st_r.graphs) and len(st.graphs) == 1
    assert torch.equal(im.sample(**kw, guidance_rescale=0.7, _use_graph=False), r7)
    both = im.sample(**kw, guidance_rescale=0.7, negative_text_embeds=neg, negative_text_masks=nmask).clone()
    assert len(st_r.graphs) == 2 and not torch.equal(both, r7)
    h = B // 2
    part = im.sample(text_embeds=emb[h:].contiguous(), text_masks=mask[h:].contiguous(), cond_scale=3., _seed=11, _sample_offset=h, guidance_rescale=0.7,
                     negative_text_embeds=neg[h:].contiguous(), negative_text_masks=nmask[h:].contiguous())
    assert torch.equal(part, both[h:])
    im.check_device_status()


@pytest.mark.parametrize("backend", GPU_ONLY)
def test_default_call_is_untouched(backend):
    """sample(guidance_rescale=0.) and sample(guidance_rescale=None) ARE sample(): same bits, no workspace, state or graph key beyond its own;
    after a rescaled call at 256^2 (a workspace of its own beside the folded one) the plain call still runs on the folded workspace and gives
    the bits it gave"""
    dev = setup(backend)
    T = 25
    im = make_imagen([64, 256], T, dev)
    emb, mask = R.synthetic_text(2, length=16, seed=7)
    kw = dict(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., _seed=11)

    def keys():
        return [(k, sk, tuple(st.graphs)) for u in im.unets for k, ws in u.engine()._ws.items() for sk, st in ws.sampler_state.items()]

    def folded():
        return [ws.cfg_fold is not None for u in im.unets for k, ws in u.engine()._ws.items() if k[-1] != "nofold"]
    a = im.sample(**kw).clone()
    before = keys()
    assert len(before) == 2 and all(sk == T and len(g) == 1 and "nofold" not in k for k, sk, g in before)
    assert folded() == [False, True]                                          # the SR stage of the cascade takes the guidance fold
    for off in (0., None, 0):
        assert torch.equal(im.sample(**kw, guidance_rescale=off), a)
    assert keys() == before
    r = im.sample(**kw, guidance_rescale=0.7).clone()
    assert not torch.equal(r, a) and r.isfinite().all()
    after = keys()
    assert after[0::2] == before and [k[-1] == "nofold" for k, _, _ in after] == [False, True, False, True]
    assert all(sk == T and len(g) == 1 and g[0][-1] == ("rescale", 0.7) for k, sk, g in after[1::2])
    assert all(ws.cfg_fold is None for u in im.unets for k, ws in u.engine()._ws.items() if k[-1] == "nofold")
    assert torch.equal(im.sample(**kw), a) and keys() == after and folded() == [False, True]
    im.check_device_status()
