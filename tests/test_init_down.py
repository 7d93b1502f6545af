"""CrossEmbed + the first level's pre-Downsample as ONE launch (mi_init_down_fwd, csrc/crossembed.hip init_down_mfma_kernel): the packer's
nine-variant composition against the sequential convolutions, the kernel against torch fp64 through the C ABI, and the engine's fused plan
against the two-launch plan (MINIMAGEN_INIT_DOWN=0)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from minimagen_amd import _lib as L, packing as P
from minimagen_amd.Unet import Unet
from oracle import restated as R
from tests import _inputs as I
from tests._backend import BACKENDS, setup
from tests.test_kernels import check_stats
from tests.test_sampler import make_imagen
from tests.test_unet import FWD_ATOL, make_unet

KS, COUT = (3, 7, 15), (4, 2, 2)


def sequential(x, ws, bs, wd, bd, c0, cin):
    """the reference's two layers: cat(conv3, conv7, conv15)(x) -> Conv2d(k4, s2, p1), in the dtype of x"""
    mid = torch.cat([F.conv2d(x, w[:, c0:c0 + cin], b, padding=(k - 1) // 2) for w, b, k in zip(ws, bs, KS)], 1)
    return F.conv2d(mid, wd, bd, stride=2, padding=1)


def variant_of(n):
    """border variant of each of n output positions: 0 first, 2 last, 1 interior"""
    v = torch.ones(n, dtype=torch.long)
    v[0], v[-1] = 0, 2
    return v


def test_composition_equals_the_sequential_convs():
    """packer alone, fp64, on the CPU: the 18 x 18 stride-2 pad-8 kernel with its 3 x 3 border variants against conv o conv, both input
    halves, down to the smallest image (every output pixel on a border) -- and the interior variant alone is NOT enough"""
    g = torch.Generator().manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    ws = [rn(co, 6, k, k) * 0.1 for k, co in zip(KS, COUT)]
    bs = [rn(co) for co in COUT]
    wd, bd = rn(8, 8, 4, 4) * 0.1, rn(8)
    for H, W in ((4, 8), (4, 4), (16, 16), (40, 24)):
        for c0, bias in ((0, True), (3, False)):
            x = rn(2, 3, H, W)
            ref = sequential(x, ws, bs if bias else [None] * 3, wd, bd if bias else None, c0, 3)
            w9, b9 = P.compose_init_down(ws, bs if bias else None, wd, bd, c0, 3)
            vy, vx = variant_of(H // 2), variant_of(W // 2)
            out = torch.empty_like(ref)
            for iy in range(3):
                for ix in range(3):
                    y = F.conv2d(x, w9[iy, ix], b9[iy, ix], stride=2, padding=8)
                    m = (vy == iy)[:, None] & (vx == ix)[None, :]
                    out[:, :, m] = y[:, :, m]
            assert (out - ref).abs().max().item() < 1e-12
            interior = F.conv2d(x, w9[1, 1], b9[1, 1], stride=2, padding=8)
            assert (interior - ref).abs().max().item() > 1e-3
            if H > 4:
                assert (interior - ref)[:, :, 1:-1, 1:-1].abs().max().item() < 1e-12


ID_CASES = [
    # B, Cin, H, W, x scale, CrossEmbed weight scale, Downsample weight scale, addend, in0_batch_mod
    (2, 3, 16, 16, 1.0, 1.0, 1.0, False, 0),            # image smaller than the window
    (2, 3, 40, 24, 1.0, 1.0, 1.0, True, 0),             # ragged tile edges; output rows that are only 8-byte aligned
    (1, 4, 72, 136, 1.0, 1.0, 1.0, False, 0),           # several tiles both ways
    (4, 3, 20, 32, 300.0, 1.0 / 64, 1.0, False, 2),     # shared input rows (guidance halves); range safety of the fp16 split
    (1, 3, 36, 40, 1.0 / 256, 30.0, 4.0, True, 0),      # range safety
    (1, 3, 4, 8, 1.0, 1.0, 1.0, False, 0),              # every output pixel on a border
]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("half", ["x", "lowres"])
@pytest.mark.parametrize("case", ID_CASES)
def test_init_down_op(backend, case, half):
    """the fused launch vs torch fp64 F.conv2d(cat(conv3, conv7, conv15)(x), Wd, bd, stride=2, padding=1) (+ addend): the gate of
    test_crossembed_matrix_core, err < 2e-5 max(1, |ref|max / 4); statistics by check_stats against the fp32 result; an all-zero image
    gives exactly the composed bias of the pixel's border variant (+ addend); two launches are bit-identical.  `lowres`: channels
    Cin .. 2 Cin - 1 of a 2 Cin-channel weight, no bias (the hoisted half).  Both tile shapes."""
    dev = setup(backend)
    lib = L.lib()
    B, Cin, H, W, xs, ces, dss, with_add, mod = case
    g = torch.Generator().manual_seed(hash(case) & 0xffff)
    rn = lambda *s_: torch.randn(*s_, generator=g)
    Bx = mod if mod else B
    Ho, Wo = H // 2, W // 2
    x = rn(Bx, Cin, H, W) * xs
    ws = [rn(co, 2 * Cin, k, k) * 0.1 * ces for k, co in zip(KS, COUT)]
    bs = [rn(co) * xs * ces for co in COUT]
    wd, bd = rn(8, 8, 4, 4) * 0.1 * dss, rn(8) * xs * ces * dss
    add = rn(B, 8, Ho, Wo) * xs * ces * dss if with_add else None
    x_half = half == "x"
    c0 = 0 if x_half else Cin
    w9, b9 = P.compose_init_down(ws, bs if x_half else None, wd, bd, c0, Cin)
    tab, exp, b32 = P.pack_init_down_mfma(w9, b9)
    tabd, b32d = tab.to(dev), b32.to(dev)
    ref = sequential(x.repeat(B // Bx, 1, 1, 1).double(), [w.double() for w in ws], [b.double() if x_half else None for b in bs],
                     wd.double(), bd.double() if x_half else None, c0, Cin)
    if with_add:
        ref = ref + add.double()
    zero_ref = (b32[variant_of(Ho)][:, variant_of(Wo)].permute(2, 0, 1) if x_half else torch.zeros(8, Ho, Wo)).expand(B, -1, -1, -1)
    if with_add:
        zero_ref = zero_ref + add
    addd = add.to(dev) if with_add else None
    for cfg in (0, 1):
        nt = lib.mi_init_down_tiles(cfg, H, W)
        assert nt == -(-Ho // 8) * -(-Wo // (64, 32)[cfg])
        outs = []
        for zero in (False, False, True):
            xd = (torch.zeros_like(x) if zero else x).to(dev)
            p = L.MiInitDownParams()
            p.B, p.H, p.W = B, H, W
            p.in0, p.C0, p.in0_batch_mod = xd.data_ptr(), Cin, mod
            p.n_kernels = 3
            for i in range(3):
                p.ksize[i], p.cout[i] = KS[i], COUT[i]
            p.Cout, p.w_tab, p.w_exp, p.bias9 = 8, tabd.data_ptr(), exp, (b32d.data_ptr() if x_half else 0)
            p.addend = addd.data_ptr() if with_add else 0
            out = torch.full((B, 8, Ho, Wo), float('nan'), device=dev)
            ost = torch.zeros(B, 8, nt, 2, dtype=torch.float64, device=dev)
            p.out, p.out_stats, p.tile_cfg = out.data_ptr(), ost.data_ptr(), cfg
            L.check(lib.mi_init_down_fwd(C.byref(p), L.current_stream()), "init_down")
            if zero:
                assert torch.equal(out.cpu(), zero_ref)
            outs.append((out.cpu(), ost.cpu()))
        (o1, s1), (o2, s2) = outs[0], outs[1]
        assert torch.equal(o1, o2) and torch.equal(s1, s2)
        err = (o1.double() - ref).abs().max().item()
        scale = max(1.0, ref.abs().max().item() / 4.0)
        print(f"init_down {case} {half} cfg {cfg}: max|d| = {err:.2e} (gate {2e-5 * scale:.2e}, |ref|max {ref.abs().max().item():.3g})")
        assert err < 2e-5 * scale
        check_stats(s1, ref.float())


def test_init_down_rejects_bad_arguments():
    setup("emu")
    lib = L.lib()
    assert lib.mi_init_down_tiles(0, 6, 6) < 0 and lib.mi_init_down_tiles(2, 8, 8) < 0 and lib.mi_init_down_tiles(1, 8, 8) == 1
    t = torch.zeros(64)
    p = L.MiInitDownParams()
    p.B, p.H, p.W, p.in0, p.C0, p.n_kernels, p.Cout, p.w_tab, p.out = 1, 8, 8, t.data_ptr(), 3, 1, 16, t.data_ptr(), t.data_ptr()
    p.ksize[0], p.cout[0] = 3, 8
    assert lib.mi_init_down_fwd(C.byref(p), None) == -3          # MI_ERR_UNSUPPORTED: 16 Downsample channels
    p.Cout, p.W = 8, 6
    assert lib.mi_init_down_fwd(C.byref(p), None) == -1          # MI_ERR_INVALID: W % 4


def _sr_inputs(dev, B=2, S=32):
    emb, mask = R.synthetic_text(B, length=12, seed=3)
    x, lr = I.seeded((B, 3, S, S), 71), I.seeded((B, 3, S, S), 72)
    tm, lt = torch.tensor([40, 7][:B]), torch.tensor([20, 20][:B])
    return x.to(dev), tm.to(dev), dict(lowres_cond_img=lr.to(dev), lowres_noise_times=lt.to(dev), text_embeds=emb.to(dev), text_mask=mask.to(dev))


@pytest.mark.parametrize("backend", BACKENDS)
def test_fused_plan_vs_two_launches(backend, monkeypatch):
    """unet1 (the SR stage of every benched cascade) at 32 x 32, B = 2, low-res conditioning and guidance: the fused plan has one launch
    fewer and agrees with the two-launch plan (MINIMAGEN_INIT_DOWN=0) to well under FWD_ATOL, the gate both plans meet against the
    goldens (measured, printed: 7.7e-06 on the emulator, 5.3e-06 on the MI355X); a B = 2 batch equals its two B = 1 shards bit for bit."""
    from minimagen_amd import engine as E
    dev = setup(backend)
    x, tm, kw = _sr_inputs(dev)
    outs, plans = [], []
    for knob in (True, False):
        monkeypatch.setattr(E, "INIT_DOWN", knob)
        u1 = make_unet("unet1", dev)
        outs.append(u1.forward_with_cond_scale(x, tm, cond_scale=3., **kw).cpu())
        ws = next(iter(u1.engine()._ws.values()))
        plans.append([name for _, _, name in ws.prog])
        if knob:
            assert ws.ce_lr.shape == (2, 8, 16, 16) and [n for _, _, n in ws.prog_pre] == ["crossembed_lowres"]
            sh = [u1.forward_with_cond_scale(x[i:i + 1], tm[i:i + 1], cond_scale=3., **{k: v[i:i + 1] for k, v in kw.items()}).cpu() for i in range(2)]
            assert torch.equal(torch.cat(sh), outs[0])
    assert len(plans[0]) == len(plans[1]) - 1 and plans[0][0] == plans[1][0] == "crossembed" and plans[1][1] == "conv"
    assert plans[0][1:] == plans[1][2:]
    d = (outs[0] - outs[1]).abs().max().item()
    print(f"fused vs two launches, unet1 32x32 B2 cfg 3: max|d| = {d:.2e}")
    assert d < FWD_ATOL


@pytest.mark.parametrize("backend", BACKENDS)
def test_captured_graph_sampling_equals_eager_with_the_fused_launch(backend):
    """a 16 -> 32 cascade sampled in T = 4 steps (of 21 trained) with guidance: HIP-graph replay == eager launches, bit for bit"""
    dev = setup(backend)
    im = make_imagen([16, 32], 21, dev)
    assert im.unets[1].engine().pack().init_down_ok
    emb, mask = R.synthetic_text(2, length=12, seed=9)
    emb, mask = emb.to(dev), mask.to(dev)
    a = im.sample(text_embeds=emb, text_masks=mask, cond_scale=3., _seed=5, sample_steps=4)
    b = im.sample(text_embeds=emb, text_masks=mask, cond_scale=3., _seed=5, sample_steps=4, _use_graph=False)
    assert torch.equal(a, b) and torch.isfinite(a).all()
