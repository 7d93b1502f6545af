"""The folded cross-attention contracted over cond_dim (variant 8 of mi_cross_attn_fwd, context fragments from mi_attn_cond_rows, per-head
tables from packing.pack_cross_attn_cond) against the oracle's unfolded CrossAttention, its fragments and step scatter, the engine plan
behind MINIMAGEN_ATTN_COND and the configurations that stay on variants 6 / 7.  max |variant 8 - variant 6| is printed wherever both run."""
import ctypes as C

import pytest
import torch

from minimagen_amd import _lib as L, packing as P
from minimagen_amd import engine as E
from minimagen_amd.Unet import Unet
from oracle import restated as R
from tests import _inputs as I
from tests._backend import BACKENDS, setup
from tests.test_kernels import check_stats
from tests.test_sampler import make_imagen
from tests.test_unet import FWD_ATOL, make_unet

HEADS = 8


def _weights(Cc, cd, q_scale=1.0, v_scale=1.0):
    """the construction of test_cross_attention_folded"""
    g = torch.Generator().manual_seed(1)
    rn = lambda *s: torch.randn(*s, generator=g)
    kv_w = rn(2 * HEADS * 64, cd) * cd ** -0.5
    kv_w[HEADS * 64:] *= v_scale                                 # the value rows
    sd = {"a.norm.gamma": 1 + 0.2 * rn(Cc), "a.norm.beta": 0.1 * rn(Cc),
          "a.to_q.weight": rn(HEADS * 64, Cc) * Cc ** -0.5 * q_scale, "a.to_kv.weight": kv_w,
          "a.null_kv": rn(2, 64), "a.to_out.0.weight": rn(Cc, HEADS * 64) * (HEADS * 64) ** -0.5,
          "a.to_out.1.gamma": 1 + 0.2 * rn(Cc), "a.to_out.1.beta": 0.1 * rn(Cc)}
    if q_scale != 1.0:
        sd["a.to_q.weight"] = sd["a.to_q.weight"] / (1.0 + 0.3 * q_scale)     # keep the logits of a usable size: the test is about the operands' range
    return sd, rn


def _cond_rows(lib, dev, frag, B2, cd, ex, rows, row0, write_null):
    fp = L.MiAttnCondParams()
    fp.B2, fp.cd, fp.JT, fp.c_exp, fp.i_exp, fp.frag = B2, cd, 17, ex["c_exp"], ex["i_exp"], frag.data_ptr()
    rows = rows.contiguous().to(dev)
    fp.c_rows, fp.c_stride_b, fp.row0, fp.nrows, fp.write_null = rows.data_ptr(), rows.shape[1] * cd, row0, rows.shape[1], write_null
    L.check(lib.mi_attn_cond_rows(C.byref(fp), L.current_stream()))
    return rows


def _attn_params(dev, sd, x, B2, Cc, HW, J):
    ap = L.MiCrossAttnParams()
    ap.B2, ap.C, ap.HW, ap.heads, ap.J = B2, Cc, HW, HEADS, J
    xd = x.to(dev)
    sdd = {k: v.to(dev) for k, v in sd.items()}
    ap.x = L.MiAct(xd.data_ptr(), Cc, 0, 0, 1.0, 0)
    ap.n1_g, ap.n1_b = sdd["a.norm.gamma"].data_ptr(), sdd["a.norm.beta"].data_ptr()
    ap.n2_g, ap.n2_b = sdd["a.to_out.1.gamma"].data_ptr(), sdd["a.to_out.1.beta"].data_ptr()
    out = torch.full(x.shape, float('nan'), device=dev)
    ost = torch.zeros(B2, Cc, -(-HW // 64), 2, dtype=torch.float64, device=dev)
    ap.out, ap.out_stats = out.data_ptr(), ost.data_ptr()
    return ap, out, ost, (xd, sdd)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", [(2, 16, 256, 8, 2), (8, 16, 200, 8, 4), (2, 16, 1100, 8, 4), (1, 8, 200, 8, 2), (1, 16, 128, 4, 2),
                                  # range safety of the fp16 splits: checkpoint weights / context rows far from unit scale
                                  (1, 16, 128, 8, 2, 256.0, 1.0 / 256, 1.0), (1, 16, 128, 8, 2, 1.0 / 64, 300.0, 40.0), (1, 8, 128, 8, 4, 30.0, 30.0, 0.01)])
def test_cross_attention_cond(backend, case):
    """variant 8 against the oracle's unfolded CrossAttention (+ residual), 3e-5 like test_cross_attention_folded: the XCD map with a
    ragged last workgroup and a partial wave (8 x 200), the 8-wave form just above the 16-wave limit (1100 tokens), C = 8, cd = 4."""
    dev = setup(backend)
    lib = L.lib()
    B2, Cc, HW, cd, ntok = case[:5]
    q_scale, v_scale, c_scale = case[5:] if len(case) > 5 else (1.0, 1.0, 1.0)
    J = 1 + ntok + 256
    sd, rn = _weights(Cc, cd, q_scale, v_scale)
    x, c = rn(B2, Cc, HW) * 1.3, rn(B2, J - 1, cd) * c_scale
    xt = x.permute(0, 2, 1)
    ref = (R.cross_attention(xt, c, sd, "a") + xt).permute(0, 2, 1).contiguous()
    mg, mv, g0, v0 = P.fold_cross_attention(sd["a.to_q.weight"], sd["a.to_kv.weight"], sd["a.to_out.0.weight"], sd["a.null_kv"], HEADS)
    cmax, xmax = float(c.abs().max()), P.layernorm_bound(sd["a.norm.gamma"], sd["a.norm.beta"], Cc)
    ex = P.attn_cond_exponents(mg, mv, g0, v0, cmax=cmax, xmax=xmax)
    assert ex is not None
    tab = P.pack_cross_attn_cond(mg, mv, g0, v0, ex["f_exp"], ex["g0_exp"], ex["mv_exp"]).to(dev)
    assert tab.shape == (HEADS, lib.mi_attn_cond_head_floats() // 256, 64, 4)
    frag = torch.zeros(B2, lib.mi_attn_cond_frag_floats(17), device=dev)
    keep = [_cond_rows(lib, dev, frag, B2, cd, ex, c[:, ntok:], 1 + ntok, 1), _cond_rows(lib, dev, frag, B2, cd, ex, c[:, :ntok], 1, 0)]
    ap, out, ost, keep2 = _attn_params(dev, sd, x, B2, Cc, HW, J)
    ap.gv, ap.head_tab, ap.variant = frag.data_ptr(), tab.data_ptr(), 8
    ap.x_exp, ap.g_exp, ap.v_exp = ex["x_exp"], ex["f_exp"] + ex["c_exp"], ex["c_exp"] + ex["mv_exp"]
    L.check(lib.mi_cross_attn_fwd(C.byref(ap), L.current_stream()))
    assert torch.isfinite(out).all()
    err = (out.cpu() - ref).abs().max().item()

    # variant 6 on the same inputs: reported, not gated
    mgd, mvd, g0d, v0d = [t.to(dev) for t in (mg, mv, g0, v0)]
    gv = torch.zeros(B2, HEADS, 18, 64, lib.mi_attn_fragment_floats(Cc), device=dev)
    x_exp, g_exp, v_exp = P.attn_f16_exponents(mg, mv, g0, v0, cmax=cmax, xmax=xmax)
    fp = L.MiAttnFoldParams()
    fp.B2, fp.C, fp.cd, fp.heads, fp.JT, fp.n_blocks, fp.frag_f16 = B2, Cc, cd, HEADS, 17, 1, 1
    fp.blk[0].g_exp, fp.blk[0].v_exp = g_exp, v_exp
    fp.blk[0].mg, fp.blk[0].mv, fp.blk[0].g0, fp.blk[0].v0, fp.blk[0].gv = mgd.data_ptr(), mvd.data_ptr(), g0d.data_ptr(), v0d.data_ptr(), gv.data_ptr()
    for rows, row0, wn in ((keep[0], 1 + ntok, 1), (keep[1], 1, 0)):
        fp.c_rows, fp.c_stride_b, fp.row0, fp.nrows, fp.write_null = rows.data_ptr(), rows.shape[1] * cd, row0, rows.shape[1], wn
        L.check(lib.mi_attn_fold_rows(C.byref(fp), L.current_stream()))
    a6, out6, _, keep3 = _attn_params(dev, sd, x, B2, Cc, HW, J)
    a6.gv, a6.variant, a6.x_exp, a6.g_exp, a6.v_exp = gv.data_ptr(), 6, x_exp, g_exp, v_exp
    L.check(lib.mi_cross_attn_fwd(C.byref(a6), L.current_stream()))
    err6 = (out6.cpu() - ref).abs().max().item()
    print(f"cross_attn cond {case}: max|d| vs oracle {err:.2e} (variant 6: {err6:.2e}), max|variant 8 - variant 6| = {(out - out6).abs().max().item():.2e}, exponents {ex}")
    assert err < 3e-5
    check_stats(ost.cpu(), ref)


def _slot(frag, b, row, lane, e):
    """half e of lane `lane` of fragment row `row` of batch row b"""
    return frag.view(torch.float16).view(frag.shape[0], -1, 64, 8)[b, row, lane, e].item()


@pytest.mark.parametrize("backend", BACKENDS)
def test_cond_fragments(backend):
    """the null indicator, the time rows and the 256 text rows land where the kernel reads them (layout in minimagen_hip.h); text rows first
    and time rows after == both at once, bit for bit; rows past J stay finite zeros"""
    dev = setup(backend)
    lib = L.lib()
    B2, cd, ntok, JT = 2, 8, 4, 17
    J = 1 + ntok + 256
    ex = dict(c_exp=3, i_exp=3)
    c = torch.randn(B2, J - 1, cd, generator=torch.Generator().manual_seed(4))
    n = lib.mi_attn_cond_frag_floats(JT)
    assert n == (17 + 9) * 64 * 4
    fa, fb = torch.zeros(B2, n, device=dev), torch.zeros(B2, n, device=dev)
    _cond_rows(lib, dev, fa, B2, cd, ex, c[:, ntok:], 1 + ntok, 1)
    _cond_rows(lib, dev, fa, B2, cd, ex, c[:, :ntok], 1, 0)
    _cond_rows(lib, dev, fb, B2, cd, ex, c, 1, 1)
    fa, fb = fa.cpu(), fb.cpu()
    assert torch.equal(fa.view(torch.int32), fb.view(torch.int32))
    assert torch.isfinite(fa.view(torch.float16).float()).all()
    cs = c * 8.0
    hi = cs.half()
    lo = (cs - hi.float()).half()
    for b, j in ((0, 1), (1, 4), (0, 5), (1, 133), (0, J - 1)):          # first / last time row, first / middle / last text row
        jt, jm = j >> 4, j & 15
        for d in range(cd):
            h, l = hi[b, j - 1, d].item(), lo[b, j - 1, d].item()
            assert _slot(fa, b, jt, jm + 16 * (d // 3), d % 3) == h and _slot(fa, b, jt, jm + 16 * (d // 3), 3 + d % 3) == h
            assert _slot(fa, b, jt, jm + 16 * (d // 2), 6 + (d & 1)) == l
            assert _slot(fa, b, JT + (jt >> 1), d + 16 * (jm >> 2), 4 * (jt & 1) + (jm & 3)) == h
            assert _slot(fa, b, JT + (jt >> 1), 8 + d + 16 * (jm >> 2), 4 * (jt & 1) + (jm & 3)) == l
        assert _slot(fa, b, jt, jm + 32, 2) == 0.0 and _slot(fa, b, jt, jm + 32, 5) == 0.0
    for b in range(B2):                                                    # the null row: the indicator alone, no value
        assert _slot(fa, b, 0, 32, 2) == 8.0 and _slot(fa, b, 0, 32, 5) == 8.0
        h16 = fa.view(torch.float16).view(B2, -1, 64, 8)[b]
        row0 = torch.cat((h16[0, 0::16].flatten(), h16[JT, :, 0][0:16]))
        assert row0.abs().sum().item() == 16.0
        for j in range(J, 16 * JT + 16):                                   # rows past J (and the pad tile of the last pair)
            jt, jm = j >> 4, j & 15
            if jt < JT:
                assert h16[jt, jm::16].abs().sum().item() == 0.0
            assert h16[JT + (jt >> 1), 16 * (jm >> 2):16 * (jm >> 2) + 16, 4 * (jt & 1) + (jm & 3)].abs().sum().item() == 0.0
    bad = L.MiAttnCondParams()
    bad.B2, bad.cd, bad.JT, bad.frag = 1, 9, 17, fa.data_ptr()
    assert lib.mi_attn_cond_rows(C.byref(bad), None) == -1               # MI_ERR_INVALID: cond_dim above 8


def _knob_unet(monkeypatch, which, dev, knob):
    monkeypatch.setattr(E, "ATTN_COND", knob)
    return make_unet(which, dev)


def _variants(u):
    return sorted({p.variant for ws in u.engine()._ws.values() for fn, p, name in ws.prog if name == "cross_attn"})


@pytest.mark.parametrize("backend", BACKENDS)
def test_step_tables_scatter_equals_forward_once(backend, monkeypatch):
    """T = 5, B2 = 4, two timesteps: prepare_step_tables + run_step (the time-token rows scattered from c_time_t) == forward_once"""
    dev = setup(backend)
    u0 = _knob_unet(monkeypatch, "unet0", dev, True)
    eng = u0.engine()
    emb, mask = R.synthetic_text(2, length=12, seed=3)
    x = I.seeded((2, 3, 16, 16), 23).to(dev)
    kw = dict(lowres_cond_img=None, lowres_noise_times=None, text_embeds=emb.to(dev), text_mask=mask.to(dev), keep=None, cond_scale=3.0)
    for t, other in ((3, 0), (1, 4)):
        eng.forward_once(x, torch.tensor([t, t]).to(dev), **kw)
        ws = eng.workspace(2, 4, 16, 16)
        assert ws.cfrag is not None and not ws.gv and _variants(u0) == [8]
        ref = ws.pred.clone()
        eng.forward_once(x, torch.tensor([other, other]).to(dev), **kw)      # the fragments and scale/shift rows now hold another timestep's
        assert not torch.equal(ws.pred, ref)
        t_state = torch.tensor([t], dtype=torch.int32, device=dev)
        eng.prepare_step_tables(ws, 5, t_state)
        assert [type(p).__name__ for _, p, _ in ws.prog_stage] == ["MiAttnCondParams"]
        eng.run_step(ws)
        assert torch.equal(ws.pred, ref)
        eng.drop_step_tables(ws, t_state)


def _fwd_inputs(which, dev, B):
    emb, mask = R.synthetic_text(B, length=12, seed=3)
    x, tm = I.seeded((B, 3, 32, 32), 71), torch.tensor([40, 7, 3, 90][:B])
    kw = dict(text_embeds=emb, text_mask=mask)
    if which == "unet1":
        kw.update(lowres_cond_img=I.seeded((B, 3, 32, 32), 72), lowres_noise_times=torch.tensor([20] * B))
    return x, tm, kw


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("which", ["unet0", "unet1"])
def test_engine_knob_on_and_off_vs_oracle(backend, which, monkeypatch):
    """golden-parameter U-Nets at 32 x 32, B = 2, conditional and null halves: MINIMAGEN_ATTN_COND on (variant 8) and off (variant 6) are
    both within FWD_ATOL of the oracle; the rows of a B = 4 call equal those of two B = 2 shards bit for bit"""
    dev = setup(backend)
    sd = I.load(f"{which}_sd.pt")
    x, tm, kw = _fwd_inputs(which, dev, 4)
    to = lambda d, s=slice(None): {k: v[s].to(dev) for k, v in d.items()}
    refs = {cdp: R.unet_forward(sd, x[:2], tm[:2], cond_drop_prob=cdp, **{k: v[:2] for k, v in kw.items()}) for cdp in (0., 1.)}
    outs = {}
    for knob in (True, False):
        u = _knob_unet(monkeypatch, which, dev, knob)
        for cdp in (0., 1.):
            o = u(x[:2].to(dev), tm[:2].to(dev), cond_drop_prob=cdp, **to(kw, slice(0, 2))).cpu()
            outs[knob, cdp] = o
            d = (o - refs[cdp]).abs().max().item()
            print(f"{which} 32x32 B2 cond_drop {cdp} ATTN_COND {int(knob)}: max|d| vs oracle = {d:.2e}")
            assert d < FWD_ATOL
        assert _variants(u) == ([8] if knob else [6])
        if knob:
            full = u(x.to(dev), tm.to(dev), cond_drop_prob=0., **to(kw)).cpu()
            hi = u(x[2:].to(dev), tm[2:].to(dev), cond_drop_prob=0., **to(kw, slice(2, 4))).cpu()
            assert torch.equal(full, torch.cat((outs[True, 0.], hi)))
    for cdp in (0., 1.):
        print(f"{which} cond_drop {cdp}: max|variant 8 - variant 6| = {(outs[True, cdp] - outs[False, cdp]).abs().max().item():.2e}")


@pytest.mark.parametrize("backend", BACKENDS)
def test_sampling_knob_on_vs_off(backend, monkeypatch):
    """base U-Net at 64^2, B = 2, T = 5 sampling steps (of the 21 trained: a schedule needs at least 20), cond_scale 3 through the captured
    graphs: knob on against knob off within the sampling gate (1e-5 mean / 1e-4 max), and a replay is bit-identical"""
    dev = setup(backend)
    emb, mask = R.synthetic_text(2, length=12, seed=9)
    emb, mask = emb.to(dev), mask.to(dev)
    outs = []
    for knob in (True, False):
        monkeypatch.setattr(E, "ATTN_COND", knob)
        im = make_imagen([64], 21, dev)
        a = im.sample(text_embeds=emb, text_masks=mask, cond_scale=3., _seed=5, sample_steps=5)
        assert _variants(im.unets[0]) == ([8] if knob else [6])
        if knob:
            assert torch.equal(a, im.sample(text_embeds=emb, text_masks=mask, cond_scale=3., _seed=5, sample_steps=5))
        outs.append(a.cpu())
    d = (outs[0] - outs[1]).abs()
    print(f"sample base 64x64 B2 T5 cfg 3, ATTN_COND on vs off: max|d| = {d.max().item():.2e}, mean|d| = {d.mean().item():.2e}")
    assert torch.isfinite(outs[0]).all() and d.max().item() < 1e-4 and d.mean().item() < 1e-5


@pytest.mark.parametrize("backend", BACKENDS)
def test_fallbacks_keep_variants_6_and_7(backend, monkeypatch):
    """reduced precision, the text-free call, C = 32 and cond_dim = 16 stay on variants 6 / 7 with the knob on, and pass"""
    dev = setup(backend)
    monkeypatch.setattr(E, "ATTN_COND", True)
    u0, sd0 = make_unet("unet0", dev), I.load("unet0_sd.pt")
    x, tm, kw = _fwd_inputs("unet0", dev, 2)
    kwd = {k: v.to(dev) for k, v in kw.items()}
    ref = R.unet_forward(sd0, x, tm, **kw)
    u0.engine().precision = "half"
    oh = u0(x.to(dev), tm.to(dev), **kwd).cpu()
    assert _variants(u0) == [7]
    d = (oh - ref).abs()
    assert d.max() < 3e-2 * ref.abs().max() and d.mean() < 3e-3 * ref.abs().max()
    u0.engine().precision = "fp32"
    o = u0(x.to(dev), tm.to(dev)).cpu()                                      # no text: the one-tile context
    assert _variants(u0) == [6, 7]
    assert (o - R.unet_forward(sd0, x, tm, text_embeds=None, text_mask=None)).abs().max() < FWD_ATOL
    assert (u0(x.to(dev), tm.to(dev), **kwd).cpu() - ref).abs().max() < FWD_ATOL
    assert _variants(u0) == [6, 7, 8]
    p = I.unet_params()["unet0"]
    for change in (dict(cond_dim=16), dict(dim=16, cond_dim=8)):            # a 16-wide context; 32 channels at the bottleneck
        torch.manual_seed(11)
        u = Unet(**{**p, **change})
        sd = {k: v.clone() for k, v in u.state_dict().items()}
        u = u.to(dev).eval()
        o = u(x.to(dev), tm.to(dev), **kwd).cpu()
        by_c = {(q.C, q.variant) for ws in u.engine()._ws.values() for fn, q, name in ws.prog if name == "cross_attn"}
        assert by_c and all(v == (8 if (c <= 16 and "dim" in change) else 6) for c, v in by_c), (change, by_c)
        assert ("dim" not in change) or (32, 6) in by_c
        assert (o - R.unet_forward(sd, x, tm, **kw)).abs().max() < FWD_ATOL * max(1.0, o.abs().max().item())
