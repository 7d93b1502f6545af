"""Classifier-free guidance folded into the U-Nets' linear tail: final_res_block.block2 of a guidance batch as ONE
B-row launch over [null rows ; conditional rows] with the weights [(1 - s) W2 ; s W2] and the weighted two-source identity residual
(csrc/conv_stripe.hip output mode 5), final_conv on B rows, the sampler tail without the combine.

Op level: the new stripe member through mi_conv_fwd against torch fp64 with the kernel family's gate 2e-5 * max(1, |ref|max / 8).
Engine level: forward_with_cond_scale with the fold and (fresh process, MINIMAGEN_CFG_FOLD=0) without it, each against the oracle under
FWD_ATOL; a changed cond_scale between sample() calls; a short guided cascade against the oracle."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from minimagen_amd import _lib as L, packing as P
from oracle import restated as R
from tests import _inputs as I
from tests._backend import BACKENDS, GPU_ONLY, ROOT, setup
from tests.test_kernels import chan_stats, check_stats

GROUPS = 4            # per half (two channels per group: the group sums cross channels, and must not cross the halves)
SS_OFF = 5

FOLD_CASES = [
    # B, H, W, cond_scale, operand scale, weight scale
    (1, 32, 256, 3.0, 1.0, 1.0),           # one statistics block
    (1, 64, 256, 7.5, 1.0, 1.0),           # a block boundary and its halo
    (8, 32, 256, 0.5, 1.0, 1.0),           # B % 8 == 0: the XCD-aware workgroup -> image map
    (1, 8, 64, 0.5, 1.0, 1.0),
    (1, 24, 64, 3.0, 1.0, 1.0),            # three blocks (H not a power of two)
    (8, 8, 64, 7.5, 1.0, 1.0),
    (8, 24, 64, 3.0, 1.0, 1.0),
    (1, 24, 64, 3.0, 1.0 / 64, 256.0),     # range safety of the fp16 split of the composed weights
]


def build_fold(case, dev, keep):
    """a 2B-row guidance batch (conditional rows first), the folded launch's parameter struct and the fp64 reference
    (1 - s) conv(a_null) + s conv(a_cond) + b + (1 - s) x_null + s x_cond, a = SiLU(scale/shift(GroupNorm(h))) per half"""
    B, H, W, s, xs, wsc = case
    g = torch.Generator().manual_seed(hash(case) & 0xffff)
    rn = lambda *s_: torch.randn(*s_, generator=g)
    h = (rn(2 * B, 8, H, W) * 1.5 + 0.3) * xs
    x = rn(2 * B, 8, H, W) * xs
    w, bias = rn(8, 8, 3, 3) * 0.2 * wsc, rn(8) * wsc
    gamma, beta = 1 + 0.2 * rn(8), 0.1 * rn(8)
    sst = rn(2 * B, SS_OFF + 16 + 3) * 0.3
    a = F.group_norm(h.double(), GROUPS, gamma.double(), beta.double(), 1e-5)
    a = F.silu(a * (sst[:, SS_OFF:SS_OFF + 8, None, None].double() + 1) + sst[:, SS_OFF + 8:SS_OFF + 16, None, None].double())
    conv = lambda t: F.conv2d(t, w.double(), None, padding=1)
    xd = x.double()
    ref = (1 - s) * conv(a[B:]) + s * conv(a[:B]) + bias.double()[None, :, None, None] + (1 - s) * xd[B:] + s * xd[:B]
    d = lambda name, t: keep.setdefault(name, t.to(dev).contiguous())
    hd, xdv, hs, ssd = d("h", h), d("x", x), d("hs", chan_stats(h)), d("ss", sst)
    p = L.MiConvParams()
    p.B, p.H, p.W = B, H, W
    p.in0 = L.MiAct(hd[B:].data_ptr(), 8, hs[B:].data_ptr(), 1, 1.0, 0)           # the null rows [B, 2B)
    p.in1 = L.MiAct(hd[:B].data_ptr(), 8, hs[:B].data_ptr(), 1, 1.0, 0)           # the conditional rows [0, B)
    p.Cout, p.ksize, p.stride, p.up2 = 8, 3, 1, 0
    wf, wexp = P.pack_conv_weight_rp(P.compose_cfg_fold(w, s))                   # [(1 - s) W ; s W], hand-composed below for comparison
    assert torch.equal(P.compose_cfg_fold(w, s), torch.cat(((1 - s) * w.double(), s * w.double()), 1))
    p.w_rp, p.w_rp_exp, p.bias = d("wf", wf).data_ptr(), wexp, d("b", bias).data_ptr()
    p.gn_groups, p.gn_gamma, p.gn_beta, p.gn_eps = 2 * GROUPS, d("g", torch.cat((gamma, gamma))).data_ptr(), d("be", torch.cat((beta, beta))).data_ptr(), 1e-5
    p.scale_shift, p.ss_stride, p.ss_off, p.ss_row1 = ssd[B:].data_ptr(), sst.shape[1], SS_OFF, -B
    p.res0 = L.MiAct(xdv[B:].data_ptr(), 8, 0, 0, 1.0 - s, 0)
    p.res1 = L.MiAct(xdv[:B].data_ptr(), 8, 0, 0, s, 0)
    return p, ref


def run(lib, p, cfg, nt, dev):
    out = torch.full((p.B, p.Cout, p.H, p.W), float('nan'), device=dev)
    ost = torch.full((p.B, p.Cout, nt, 2), float('nan'), dtype=torch.float64, device=dev)
    p.out, p.out_stats, p.tile_cfg = out.data_ptr(), ost.data_ptr(), cfg
    L.check(lib.mi_conv_fwd(C.byref(p), L.current_stream()), "mi_conv_fwd")
    return out.cpu(), ost.cpu()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", FOLD_CASES)
def test_folded_block2_member_vs_fp64(backend, case):
    dev = setup(backend)
    lib = L.lib()
    keep = {}
    p, ref = build_fold(case, dev, keep)
    B, H, W = case[:3]
    rows = lib.mi_conv_stripe_rows(C.byref(p))
    assert rows == W // 8, f"the stripe kernel does not take {case}"
    nt = H // rows
    out, ost = run(lib, p, 12, nt, dev)
    scale = max(1.0, ref.abs().max().item() / 8.0)
    err = (out.double() - ref).abs().max().item()
    print(f"folded block2 {case}: max|d| = {err:.2e} (gate {2e-5 * scale:.2e}, |ref|max {ref.abs().max().item():.3g})")
    assert err < 2e-5 * scale
    check_stats(ost, ref.float())
    # speed-only knobs: statistics blocks per workgroup, image order -- same outputs, same partial statistics, bit for bit
    for nblk in (1, 2, nt):
        if nt % nblk == 0 and nblk <= 15:
            o2, s2 = run(lib, p, 12 | (nblk << 12), nt, dev)
            assert torch.equal(o2, out) and torch.equal(s2, ost), f"{nblk} statistics blocks per workgroup change the result"
    o3, s3 = run(lib, p, 12 | 0x200, nt, dev)
    assert torch.equal(o3, out) and torch.equal(s3, ost)


def test_fold_eligibility_and_abi():
    """what the library takes (no compute, no GPU): the two members, nothing else; the tile kernels refuse the launch instead of dropping
    the second residual; the new field sits in former padding (no offset or size of mi_conv_params changed within ABI 12)"""
    setup("emu")
    lib = L.lib()
    assert L.MiConvParams.ss_row1.offset == 156 and L.MiConvParams.scale_shift.offset == 160
    assert lib.mi_struct_size(1) == C.sizeof(L.MiConvParams) == 360

    def probe(W=256, H=64, **kw):
        p = L.MiConvParams()
        p.B, p.H, p.W, p.Cout, p.ksize, p.stride, p.gn_groups, p.w_rp = 2, H, W, 8, 3, 1, 8, 1
        p.in0, p.in1 = L.MiAct(1, 8, 1, 1, 1.0, 0), L.MiAct(1, 8, 1, 1, 1.0, 0)
        p.res0, p.res1 = L.MiAct(1, 8, 0, 0, -2.0, 0), L.MiAct(1, 8, 0, 0, 3.0, 0)
        p.ss_row1 = -2
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    assert lib.mi_conv_stripe_rows(C.byref(probe())) == 32
    assert lib.mi_conv_stripe_rows(C.byref(probe(W=64, H=24))) == 8
    assert lib.mi_conv_stripe_rows(C.byref(probe(W=128))) == 0 and lib.mi_conv_stripe_rows(C.byref(probe(W=32, H=32))) == 0
    assert lib.mi_conv_stripe_rows(C.byref(probe(gn_groups=0))) == 0
    assert lib.mi_conv_stripe_rows(C.byref(probe(res1=L.MiAct(1, 16, 0, 0, 3.0, 0)))) == 0
    assert lib.mi_conv_stripe_rows(C.byref(probe(in0=L.MiAct(1, 16, 1, 1, 1.0, 0)))) == 0
    q = probe(in1=L.MiAct(0, 0, 0, 0, 0.0, 0), res1=L.MiAct(0, 0, 0, 0, 0.0, 0))
    assert lib.mi_conv_stripe_rows(C.byref(q)) == 0                    # a second scale/shift row without a second input
    q.ss_row1 = 0
    assert lib.mi_conv_stripe_rows(C.byref(q)) == 32                   # ... which is the plain 8 -> 8 + identity residual member
    p = probe(tile_cfg=6, out=1)
    assert lib.mi_conv_fwd(C.byref(p), None) == -3                     # MI_ERR_UNSUPPORTED on the tile kernel


# ---------------------------------------------------------------------------------------------------------------- engine level
_FWD = """
import sys, torch
sys.path.insert(0, {root!r})
from tests._backend import setup
from tests.test_cfg_fold import fwd_inputs
from tests.test_unet import make_unet
dev = setup("gpu")
x, tm, kw = fwd_inputs({which!r})
u = make_unet({which!r}, dev)
o = u.forward_with_cond_scale(x.to(dev), tm.to(dev), cond_scale=3., **{{k: v.to(dev) for k, v in kw.items()}}).cpu()
ws = next(iter(u.engine()._ws.values()))
assert ws.cfg_fold is None and ws.pred.shape[0] == 2
torch.save(o, {out!r})
"""


def fwd_inputs(which):
    S = 64 if which == "unet0" else 256
    emb, mask = R.synthetic_text(1, length=24, seed=11)
    x, tm = I.seeded((1, 3, S, S), 81), torch.tensor([37])
    kw = dict(text_embeds=emb, text_mask=mask)
    if which == "unet1":
        kw.update(lowres_cond_img=I.seeded((1, 3, S, S), 82), lowres_noise_times=torch.tensor([20]))
    return x, tm, kw


@pytest.mark.parametrize("backend", GPU_ONLY)
@pytest.mark.parametrize("which", ["unet0", "unet1"])
def test_forward_with_cond_scale_folded_and_unfolded_vs_oracle(backend, which, monkeypatch, tmp_path):
    """unet_0 at 64^2 (folded on request: MINIMAGEN_CFG_FOLD=2) and unet_1 at 256^2 (folded by default), B = 1, cond_scale 3: with the
    fold, and without it in a fresh process, each under FWD_ATOL of the oracle.  The on-vs-off difference is printed, not gated
    (measured on the MI355X: profiles/r16_cfg_fold.txt)."""
    from minimagen_amd import engine as E
    from tests.test_unet import FWD_ATOL, make_unet
    dev = setup(backend)
    monkeypatch.setattr(E, "CFG_FOLD", 2 if which == "unet0" else 1)
    x, tm, kw = fwd_inputs(which)
    u = make_unet(which, dev)
    on = u.forward_with_cond_scale(x.to(dev), tm.to(dev), cond_scale=3., **{k: v.to(dev) for k, v in kw.items()}).cpu()
    ws = next(iter(u.engine()._ws.values()))
    assert ws.cfg_fold is not None and ws.cfg_fold.scale == 3.0 and ws.pred.shape[0] == 1 and ws.B2 == 2
    out = str(tmp_path / "off.pt")
    env = dict(os.environ, MINIMAGEN_CFG_FOLD="0")
    subprocess.run([sys.executable, "-c", _FWD.format(root=ROOT, which=which, out=out)], check=True, env=env, cwd=ROOT, timeout=300)
    off = torch.load(out)
    ref = R.unet_forward_with_cond_scale(I.load(f"{which}_sd.pt"), x, tm, cond_scale=3., **kw)
    d_on, d_off, d = (on - ref).abs().max().item(), (off - ref).abs().max().item(), (on - off).abs().max().item()
    print(f"{which} cond_scale 3 B=1: folded vs oracle {d_on:.2e}, unfolded vs oracle {d_off:.2e}, folded vs unfolded {d:.2e} (|ref|max {ref.abs().max().item():.3g})")
    assert d_on < FWD_ATOL and d_off < FWD_ATOL


_CASCADE = {}
STEPS = dict(sample_steps=5, sampler="ddpm")


def _cascade(dev):
    """the 64 -> 256 cascade of the tests below, five steps per stage (strided DDPM over a 25-step schedule: GaussianDiffusion takes no
    schedule shorter than 20), B = 2, with its first cond_scale 3 sample (computed once)"""
    if not _CASCADE:
        from tests.test_sampler import make_imagen
        im = make_imagen([64, 256], 25, dev)
        emb, mask = R.synthetic_text(2, length=24, seed=9)
        _CASCADE.update(im=im, emb=emb, mask=mask)
        _CASCADE["first"] = im.sample(text_embeds=emb.to(dev), text_masks=mask.to(dev), cond_scale=3., _noise=R.make_randn(21), **STEPS)
    return _CASCADE


@pytest.mark.parametrize("backend", GPU_ONLY)
def test_short_guided_cascade_vs_oracle(backend):
    """64 -> 256, five steps per stage, B = 2, cond_scale 3, injected noise, against the oracle's U-Net in the restated loop of
    tests/test_sample_steps.py: the gate of the cascade golden (max|d| < 1e-4, mean|d| < 1e-5 on [0, 1] images)"""
    from tests.test_sample_steps import restated_sample
    dev = setup(backend)
    c = _cascade(dev)
    ws = [w for w in c["im"].unets[1].engine()._ws.values() if w.B2 == 2 * w.B]
    assert ws and all(w.cfg_fold is not None and w.pred.shape[0] == w.B for w in ws)
    ref = restated_sample([I.load("unet0_sd.pt"), I.load("unet1_sd.pt")], [64, 256], 25, 5, "ddpm", None, text_embeds=c["emb"], text_masks=c["mask"],
                          cond_scale=3., randn=R.make_randn(21))
    d = (c["first"].cpu() - ref).abs()
    print(f"folded cascade 64->256, 5 steps, cs=3 B=2 vs oracle: max|d| = {d.max():.2e}, mean|d| = {d.mean():.2e}")
    assert c["first"].shape == (2, 3, 256, 256) and d.max() < 1e-4 and d.mean() < 1e-5, (d.max(), d.mean())


@pytest.mark.parametrize("backend", GPU_ONLY)
def test_changing_cond_scale_between_calls(backend):
    """3 -> 5 -> 3 on one Imagen: the per-scale packed weights and the graph keys -- the first and the third image are equal bit for bit"""
    dev = setup(backend)
    c = _cascade(dev)
    im, emb, mask = c["im"], c["emb"].to(dev), c["mask"].to(dev)
    a = im.sample(text_embeds=emb, text_masks=mask, cond_scale=3., _seed=5, **STEPS)
    b = im.sample(text_embeds=emb, text_masks=mask, cond_scale=5., _seed=5, **STEPS)
    a2 = im.sample(text_embeds=emb, text_masks=mask, cond_scale=3., _seed=5, **STEPS)
    assert torch.equal(a, a2) and not torch.equal(a, b)
    pk = im.unets[1].engine().packed()
    assert sorted(pk.cfg_fold_w) == [1.0, 3.0, 5.0]                       # the workspace default and the two scales, each packed once
