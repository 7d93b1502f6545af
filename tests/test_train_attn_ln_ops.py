"""Op-level fp64 parity of the two training kernel files that sit on every BASELINE training step around the bottleneck cross-attention,
called through the C ABI directly:

A  mi_folded_attn_fwd / mi_folded_attn_bwd (attn_train.hip): every matrix-core instantiation the dispatch can pick at C = 16 (forward and dq
   <TT, NW> x NJT_MAX, dkv <NJT_MAX, NW>), the VALU kernels at C = 8 / 16 / 32 up to their capacity edges, oh = NULL, explicit token chunks
   (ragged and empty ones), six kinds of masks, three score regimes (flat; maxima that rise tile after tile; maxima that fall), rejections;
B  mi_layernorm_fwd / mi_layernorm_bwd (train_ln.hip): both forms at every row count around a workgroup, rows_per = 2 in both backward
   kernels, idle workgroups, the strided loop of the reduction, optional arguments, ill-conditioned data, rejections.

Every reference is fp64 torch autograd on the CPU; the gate is test_attn_ops' yardstick per output tensor: 4 x the error of the same formula
in fp32 torch ops on the CPU + 4 fp32 ulps of max |ref| (within_yardstick).  Outputs and workspaces are pre-filled with NaN and followed by
a canary, every launch runs twice and must repeat its bits, inputs must come back bit-unchanged.  The attention backward departs from that gate in two
places, both named where they are defined: WIDENED (a wider multiplier for single outputs of single cases, twice the measured ratio, with
the reason) and single_live_floor (dS = dP - D is an exact zero with one live context row; the matrix-core kernels evaluate its two halves in
two orders; the VALU kernels must return exact zeros).  test_every_launch_form_is_reached derives
the launch forms of all cases from the dispatch rules restated here (attn_forms, ln_forms) and fails when a form is no longer covered."""
import ctypes as C
import functools
import os

import pytest
import torch
import torch.nn.functional as F

from minimagen_amd import _lib as L, train_ops
from tests._backend import BACKENDS, setup
from tests.test_block_bwd_ops import bits, canary_intact, f32_ulp, guarded, within_yardstick

MI_ERR_INVALID, MI_ERR_UNSUPPORTED = -1, -3
LN2 = 0.6931471805599453
EPS = 1e-5
AT_CAP = 6144                               # floats of one (image, head)'s keys in LDS (attn_train.hip)
FLAT_GATE = 3e-5                            # the gate of test_training's tests of the same kernels: err <= 3e-5 max(1, |ref|max)


def host(flat, view):
    flat = flat.cpu()
    return flat, flat[:view.numel()].view(view.shape)


def old_flat_gate(what, out, ref):
    err, refmax = (out.double() - ref).abs().max().item(), ref.abs().max().item()
    assert err <= FLAT_GATE * max(1.0, refmax), (what, "the 3e-5 gate of test_training", err, refmax)


def gate(what, out, ref, yard_out, mult=4.0, floor=0.0):
    """within_yardstick, with another multiplier (WIDENED) or an absolute bound in the place of a yardstick that is exactly zero (single_live_floor)"""
    if mult == 4.0 and floor == 0.0:
        return within_yardstick(what, out, ref, yard_out)
    assert torch.isfinite(out).all(), f"{what}: output not finite / not fully written"
    err, yard, refmax = (out.double() - ref).abs().max().item(), (yard_out.double() - ref).abs().max().item(), ref.abs().max().item()
    tol = mult * yard + 4.0 * f32_ulp(refmax) + floor
    print(f"{what}: max|d| {err:.2e}, yardstick {yard:.2e}, |ref|max {refmax:.3g}, kernel error / yardstick {err / max(yard, 1e-30):.2f}, multiplier {mult:g}, "
          f"absolute bound {floor:.2e}, error / tolerance {err / tol:.2f}")
    assert err <= tol, (what, err, yard, mult, floor, tol)


# ---------------------------------------------------------------------------------------------------------------------------------
# A. folded attention

def attn_forms(B, n, H, J, Cc, valu=False, with_oh=True):
    """the kernels mi_folded_attn_fwd + mi_folded_attn_bwd launch for a shape: folded_dispatch and launch_folded_*_mfma of attn_train.hip restated"""
    mfma = Cc == 16 and J <= 16 * 24 and not valu
    wg256 = -(-n // 256) * B
    tw = "2,8" if wg256 >= 512 else ("2,4" if 2 * wg256 >= 512 else "1,4")
    njt = 17 if J <= 16 * 17 else 24
    fwd = f"fwd<{tw}>/{njt}" if mfma else f"fwd-valu{Cc}"
    dq = f"dq<{tw}>/{njt}" if mfma and with_oh else f"dq-valu{Cc}"
    dkv = ("dkv<12,4>" if J <= 192 else ("dkv<18,6>" if J <= 288 else "dkv<24,8>")) if mfma else f"dkv-valu{Cc}"
    return (fwd, dq, dkv, "dq+oh" if with_oh else "dq-oh")


def A(name, B, n, H, J, forms, Cc=16, mask="none", regimes=("flat",), nchunk=1, valu=False, oh=True):
    return dict(name=name, B=B, n=n, H=H, J=J, C=Cc, mask=mask, regimes=regimes, nchunk=nchunk, valu=valu, oh=oh, forms=forms)


ALL3 = ("flat", "asc12", "asc60", "desc12", "desc60")
M14, M24, M28 = "<1,4>", "<2,4>", "<2,8>"


def mf(tw, njt, dkv):
    return (f"fwd{tw}/{njt}", f"dq{tw}/{njt}", f"dkv<{dkv}>", "dq+oh")


def vf_(Cc, oh=True):
    return (f"fwd-valu{Cc}", f"dq-valu{Cc}", f"dkv-valu{Cc}", "dq+oh" if oh else "dq-oh")


ATTN_CASES = [
    # fwd / dq <1,4> at NJT 17; dkv <12,4> with idle waves
    A("1,4-j37", 2, 70, 3, 37, mf(M14, 17, "12,4"), mask="prefix", nchunk=2),
    A("1,4-one", 1, 1, 1, 1, mf(M14, 17, "12,4")),
    A("1,4-j5", 1, 17, 1, 5, mf(M14, 17, "12,4"), mask="last"),
    # fwd / dq <1,4> at NJT 24; dkv <24,8> at the cap; all score regimes (24 context tiles) over four images: the regime properties are medians over
    # the tokens, and 66 tokens behind one direction u are too few for a stable one
    A("1,4-j384", 1, 33, 2, 384, mf(M14, 24, "24,8")),
    A("1,4-j384-regimes", 4, 33, 2, 384, mf(M14, 24, "24,8"), regimes=ALL3),
    A("2,4-j20", 256, 150, 2, 20, mf(M24, 17, "12,4"), mask="prefix"),
    A("2,4-j273", 256, 40, 1, 273, mf(M24, 24, "18,6"), mask="suffix"),
    A("2,4-j289", 256, 40, 1, 289, mf(M24, 24, "24,8"), mask="middle"),
    A("2,8-j272", 512, 40, 2, 272, mf(M28, 17, "18,6"), mask="prefix"),
    A("2,8-two-wg", 256, 300, 2, 20, mf(M28, 17, "12,4"), nchunk=2),          # two token workgroups, the second ragged (44 tokens)
    A("2,8-j384", 512, 20, 1, 384, mf(M28, 24, "24,8"), regimes=ALL3),
    # dkv boundaries
    A("dkv-j16", 2, 130, 2, 16, mf(M14, 17, "12,4")),
    A("dkv-j17", 2, 130, 2, 17, mf(M14, 17, "12,4"), mask="suffix"),
    A("dkv-j192", 2, 130, 2, 192, mf(M14, 17, "12,4"), mask="middle"),
    A("dkv-j193", 2, 130, 2, 193, mf(M14, 17, "18,6"), mask="first"),
    A("dkv-j288", 2, 130, 2, 288, mf(M14, 24, "18,6"), mask="last"),
    # masks at one shape (J = 37: three context tiles, the last ragged)
    *[A(f"mask-{m}", 2, 70, 3, 37, mf(M14, 17, "12,4"), mask=m) for m in ("suffix", "middle", "first", "last", "none")],
    # explicit token chunks: per = 130, 65, 44, 19; n = 5 in 4 chunks of 2: the last is empty
    *[A(f"nchunk{c}", 2, 130, 2, 37, mf(M14, 17, "12,4"), mask="prefix", nchunk=c) for c in (1, 2, 3, 7)],
    A("nchunk-empty", 2, 5, 2, 37, mf(M14, 17, "12,4"), nchunk=4),
    A("nchunk-empty-c8", 2, 5, 2, 37, vf_(8), Cc=8, nchunk=4),
    # VALU kernels
    A("valu8-j261", 2, 70, 2, 261, vf_(8), Cc=8, regimes=ALL3),
    A("valu8-j768", 1, 40, 1, 768, vf_(8), Cc=8, mask="suffix", nchunk=2),    # the cap: a 768-work-item dkv block
    A("valu32-j20", 3, 129, 2, 20, vf_(32), Cc=32, mask="prefix", nchunk=3),
    A("valu32-j192", 1, 40, 2, 192, vf_(32), Cc=32, regimes=ALL3),             # the cap
    *[A(f"valu8-n{n}", 1, n, 2, 37, vf_(8), Cc=8, mask=m, nchunk=c) for n, m, c in ((1, "none", 1), (255, "suffix", 2), (256, "middle", 1), (257, "first", 3))],
    *[A(f"valu8-mask-{m}", 2, 70, 2, 37, vf_(8), Cc=8, mask=m) for m in ("prefix", "last")],
    A("valu16-env", 2, 70, 3, 37, vf_(16), mask="suffix", valu=True, nchunk=2),
    A("valu16-env-n257", 1, 257, 2, 261, vf_(16), mask="middle", valu=True),
    # oh = NULL: the VALU dq kernel recomputes D, at C = 16 after a matrix-core forward
    A("no-oh-c8", 2, 70, 2, 37, vf_(8, False), Cc=8, mask="prefix", oh=False),
    A("no-oh-c16", 2, 70, 3, 37, ("fwd<1,4>/17", "dq-valu16", "dkv<12,4>", "dq-oh"), mask="middle", oh=False, nchunk=2),
    A("no-oh-c16-j300", 1, 33, 2, 300, ("fwd<1,4>/24", "dq-valu16", "dkv<24,8>", "dq-oh"), oh=False, regimes=("flat", "asc60")),
]
EMU_SLOW = ()                               # cases above ~20 s on the emulator: none, the slowest (2,8-j272) takes 7 s

# Wider multipliers, C.3 of the issue: (case, regime, output) -> twice the larger measured kernel error / yardstick (MI355X | emulator).
# The reason is the same for all of them.  The backward does not keep the probabilities, it recomputes p = exp2(s2 - lse2) from the saved
# logsumexp in the log2 domain (the file's header): lse2 is rounded when it is stored, q log2(e) per component, and the difference again --
# roundings at the magnitude of lse2 that torch's exp(s - max) / sum does not have.  They weigh most where lse2 is large against the scores
# behind a probability: J = 768 flat scores (lse2 ~ 10, p ~ 1e-3: p good to 7e-7 against torch's 1e-7) and score maxima of 73 (lse2 ~ 105).
WIDENED = {("1,4-j384-regimes", "desc60", "dvf"): 2 * 4.53,      # 4.52 | 4.53   dkv <24,8>, score maxima of 73 at the FIRST context rows
           ("valu8-j768", "flat", "dkf"): 2 * 6.76,                # 6.76 | 5.07   VALU dkv at the J * C cap
           ("valu8-j768", "flat", "dvf"): 2 * 7.00}                # 5.31 | 7.00



def make_mask(kind, B, J):
    """[B][J] bool, at least one live row per image; None for "none" """
    j = torch.arange(J)[None, :]
    b = torch.arange(B)[:, None]
    if kind == "none":
        return None
    if kind == "prefix":                    # 2 .. J live rows
        assert J > 2
        return j < (J - (5 * b + 3) % (J - 1))
    if kind == "suffix":                    # the leading >= 16 rows (a whole matrix-core tile, two VALU blocks) are masked; J = 17: one live row
        assert J > 16
        return j >= 16 + (3 * b) % max(1, J - 17)
    if kind == "middle":                    # one fully masked 16-row tile in the middle
        assert J > 32
        return ((j < 16) | (j >= 32)).expand(B, J).clone()
    if kind == "first":
        return (j == 0).expand(B, J).clone()
    if kind == "last":
        return (j == J - 1).expand(B, J).clone()
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def attn_case(B, n, H, J, Cc, mask_kind, regime, nchunk):
    """inputs, the fp64 results and the fp32 yardstick of one case (shared by both backends): out, lse (natural log), oh, dsum, dq, and dkf / dvf
    per token chunk (gy zeroed outside the chunk's tokens: every out_i depends on q_i alone, so that is the chunk's exact share) and in total"""
    g = torch.Generator().manual_seed(B * 1000003 + n * 1009 + J * 17 + Cc + len(regime))
    rn = lambda *s: torch.randn(*s, generator=g)
    a = float(regime[-2:]) if regime != "flat" else 0.0
    u = F.normalize(rn(Cc), dim=0)
    ramp = torch.linspace(0, 1, J) if J > 1 else torch.zeros(1)
    if regime.startswith("desc"):
        ramp = ramp.flip(0)
    q = a ** 0.5 * u + 0.5 * rn(B, n, Cc)
    kf = a ** 0.5 * ramp[:, None] * u + 0.3 * rn(B, H, J, Cc)
    vf, gy = rn(B, H, J, Cc), rn(B, n, Cc)
    mask = make_mask(mask_kind, B, J)
    if mask is not None:                    # removed rows hold 1e4: a leak is far off
        dead = ~mask[:, None, :, None].expand(B, H, J, Cc)
        kf, vf = kf.masked_fill(dead, 1e4), vf.masked_fill(dead, 1e4)
    per = -(-n // nchunk)
    out = dict(q=q, kf=kf, vf=vf, gy=gy, mask=mask)
    for key, dt in (("ref", torch.float64), ("yard", torch.float32)):
        ql, kl, vl = (t.to(dt).requires_grad_() for t in (q, kf, vf))
        sim = torch.einsum('bnc,bhjc->bhnj', ql, kl)
        if mask is not None:
            sim = sim.masked_fill(~mask[:, None, None, :], -torch.finfo(torch.float32).max)
        oh = torch.einsum('bhnj,bhjc->bnhc', sim.softmax(-1), vl)
        o = oh.sum(2)
        r = dict(out=o.detach(), oh=oh.detach(), lse=torch.logsumexp(sim, -1).permute(0, 2, 1).detach().contiguous(),
                 dsum=(gy.to(dt)[:, :, None, :] * oh.detach()).sum(-1),                                                    # D = dO . O_h, the form with oh
                 dsum_p=(sim.detach().softmax(-1) * torch.einsum('bnc,bhjc->bhnj', gy.to(dt), vl.detach())).sum(-1).permute(0, 2, 1))   # D = sum_j p_j dP_j, without
        dk, dv = [], []
        for c in range(nchunk):
            gc = torch.zeros(B, n, Cc, dtype=dt)
            gc[:, c * per:(c + 1) * per] = gy[:, c * per:(c + 1) * per].to(dt)
            gr = torch.autograd.grad(o, (kl, vl), gc, retain_graph=True)
            dk.append(gr[0]), dv.append(gr[1])
        r["dq"], dkt, dvt = torch.autograd.grad(o, (ql, kl, vl), gy.to(dt))
        r["dkf"], r["dvf"] = torch.stack(dk), torch.stack(dv)
        r["dkf_sum"], r["dvf_sum"] = dkt, dvt
        if key == "ref" and regime != "flat":
            r["sim"] = sim.detach()
        out[key] = r
    return out


def single_live_floor(case, Cc):
    """Images with ONE live context row (masks "first" / "last", J = 1): p = 1, so dS = p (dP - D) with D = dO . O_h = dO . vf_live = dP is zero in
    exact arithmetic, and so are dq and dkf; fp64 autograd and fp32 torch both return exact zeros (softmax's backward subtracts the very number it
    multiplied), which leaves the yardstick without a scale.  The matrix-core kernels take D from the saved oh with an fma chain per lane and two
    cross-lane additions, and dP from four v_mfma_f32_16x16x4_f32 steps: two correctly rounded evaluations of the same C-term dot product in two
    orders, each within C u sum_c |dO_c vf_c| of it (u = 2^-24).  What is left is bounded term by term by
        |dq_ic|  <= 2 C u sum_h (sum_c' |dO_ic' vf_hc'|) |kf_hc|,       |dkf_hc| <= 2 C u sum_i (sum_c' |dO_ic' vf_hc'|) |q_ic|
    -- from the inputs and the number format alone.  It stands in for the (zero) yardstick of dq / dkf of the matrix-core kernels for these masks
    only; the VALU kernels evaluate both in one order, and the test asserts that they return exact zeros.
    -> (bound for dq, bound for dkf, the single-live images)"""
    mask, q, kf, vf, gy = case["mask"], case["q"].double(), case["kf"].double(), case["vf"].double(), case["gy"].double()
    B, H, J, _ = kf.shape
    live = torch.ones(B, J, dtype=torch.bool) if mask is None else mask
    one = (live.sum(1) == 1).nonzero().flatten()
    if one.numel() == 0:
        return 0.0, 0.0, one
    row = live[one].double().argmax(1)
    kl, vl = kf[one, :, row].abs(), vf[one, :, row].abs()                                              # [B'][H][C]
    gy, q = gy[one], q[one]
    gv = torch.einsum('bnc,bhc->bhn', gy.abs(), vl)
    u2c = 2.0 * Cc * 2.0 ** -24
    return u2c * torch.einsum('bhn,bhc->bnc', gv, kl).max().item(), u2c * torch.einsum('bhn,bnc->bhc', gv, q.abs()).max().item(), one


def check_regime(what, sim, regime, tile):
    """the score regime the case claims, from its own fp64 scores [B][H][n][J]: how often a tile's maximum rises above the running maximum
    (the online softmax then rescales l and acc), and how peaked the softmax is"""
    if regime == "flat":
        return
    J = sim.shape[-1]
    nt = -(-J // tile)
    pad = F.pad(sim, (0, nt * tile - J), value=float("-inf")).reshape(*sim.shape[:-1], nt, tile).amax(-1)
    rises = (pad[..., 1:] > pad.cummax(-1).values[..., :-1]).sum(-1).flatten().double()
    med, top = rises.median().item(), sim.softmax(-1).amax(-1).flatten().median().item()
    print(f"{what}: score max {sim.max().item():.1f}, median rises {med:.0f} of {nt - 1} later tiles of {tile}, median top probability {top:.2f}")
    if regime.startswith("asc"):             # half of the nt - 1 tiles that can rise at all: the first one has nothing to rise above (19 tiles at J = 300: "13 of 18")
        assert med >= (nt - 1) / 2, (what, "the maximum does not keep rising", med, nt)
    else:
        assert med == 0, (what, "the maximum rises in a descending regime", med)
    if regime.endswith("60"):
        assert top > 0.3, (what, "a = 60 should be peaked", top)


def attn_params(d, bufs, keep, m8, nchunk):
    p = L.MiFoldedAttnParams()
    p.B, p.n, p.H, p.J, p.C, p.nchunk = d["B"], d["n"], d["H"], d["J"], d["C"], nchunk
    p.q, p.kf, p.vf, p.dout, p.mask = keep["q"].data_ptr(), keep["kf"].data_ptr(), keep["vf"].data_ptr(), keep["gy"].data_ptr(), L.ptr(m8)
    for k, (_, view) in bufs.items():
        setattr(p, k, view.data_ptr())
    return p


def run_attn(dev, d, case):
    """forward then backward on guarded buffers -> every output and workspace on the host"""
    lib = L.lib()
    B, n, H, J, Cc, nchunk = d["B"], d["n"], d["H"], d["J"], d["C"], d["nchunk"]
    keep = {k: case[k].to(dev).contiguous() for k in ("q", "kf", "vf", "gy")}
    m8 = None if case["mask"] is None else case["mask"].to(torch.uint8).to(dev).contiguous()
    shapes = dict(out=(B, n, Cc), lse=(B, n, H), dsum=(B, n, H), dq=(B, n, Cc), dkf=(nchunk, B, H, J, Cc), dvf=(nchunk, B, H, J, Cc))
    if d["oh"]:
        shapes["oh"] = (B, n, H, Cc)
    bufs = {k: guarded(s, torch.float32, dev) for k, s in shapes.items()}
    p = attn_params(d, bufs, keep, m8, nchunk)
    if d["valu"]:
        os.environ["MI_FOLDED_ATTN_VALU"] = "1"
    try:
        L.check(lib.mi_folded_attn_fwd(C.byref(p), L.current_stream()), "mi_folded_attn_fwd")
        L.check(lib.mi_folded_attn_bwd(C.byref(p), L.current_stream()), "mi_folded_attn_bwd")
    finally:
        os.environ.pop("MI_FOLDED_ATTN_VALU", None)
    res = {}
    for k, (flat, view) in bufs.items():
        flat, res[k] = host(flat, view)
        assert canary_intact(flat), f"the elements after {k} were overwritten"
    for k in keep:
        assert torch.equal(bits(keep[k].cpu()), bits(case[k])), f"the input {k} was written"
    if m8 is not None:
        assert torch.equal(m8.cpu(), case["mask"].to(torch.uint8)), "the mask was written"
    return res


ATTN_RUNS = [(d, r) for d in ATTN_CASES for r in d["regimes"]]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("d,regime", ATTN_RUNS, ids=[f"{d['name']}-{r}" for d, r in ATTN_RUNS])
def test_folded_attention_direct(backend, d, regime):
    """mi_folded_attn_fwd + mi_folded_attn_bwd against fp64 autograd of out = sum_h softmax_j(q . kf_h) vf_h (mask as masked_fill(-finfo.max)):
    out, lse (from the log2 domain) against the fp64 logsumexp per (token, head), oh against the per-head output, dsum against dO . O_h, dq, and
    dkf / dvf PER CHUNK PARTIAL as well as summed, each within the fp32 yardstick; rows the mask removes are exact zeros in every partial, an
    empty chunk is all zeros.  The launch forms the shape selects are derived from the dispatch rules and must be the ones the case is listed for."""
    B, n, H, J, Cc, nchunk = d["B"], d["n"], d["H"], d["J"], d["C"], d["nchunk"]
    assert attn_forms(B, n, H, J, Cc, d["valu"], d["oh"]) == d["forms"], (d["name"], "the dispatch no longer sends this shape to the form it is listed for")
    assert J * Cc <= AT_CAP
    if backend == "emu" and d["name"] in EMU_SLOW:
        pytest.skip("emulator time")
    dev = setup(backend)
    what = f"folded-attn {backend} {d['name']} {regime} B{B} n{n} H{H} J{J} C{Cc} nchunk{nchunk}"
    case = attn_case(B, n, H, J, Cc, d["mask"], regime, nchunk)
    ref, yard = case["ref"], case["yard"]
    check_regime(what, ref.get("sim"), regime, 16 if d["forms"][0].startswith("fwd<") else 8)
    runs = [run_attn(dev, d, case) for _ in range(2)]
    for k in runs[0]:
        assert torch.equal(bits(runs[0][k]), bits(runs[1][k])), f"{what}: {k} differs between two runs"
    r = runs[0]
    r["lse"] = r["lse"].double() * LN2
    fl_dq, fl_dkf, single = single_live_floor(case, Cc)
    mfma_dq, mfma_dkv = d["forms"][1].startswith("dq<"), d["forms"][2].startswith("dkv<")
    one = dict(dq=fl_dq if mfma_dq else 0.0, dkf=fl_dkf if mfma_dkv else 0.0)
    mult = lambda k: WIDENED.get((d["name"], regime, k), 4.0)
    for k in ("out", "lse", "dsum", "dq") + (("oh",) if d["oh"] else ()):
        kr = "dsum_p" if k == "dsum" and not d["oh"] else k
        gate(f"{what} {k}", r[k], ref[kr], yard[kr], mult(k), one.get(k, 0.0))
    per = -(-n // nchunk)
    for k in ("dkf", "dvf"):
        assert torch.isfinite(r[k]).all(), f"{what}: {k} not fully written"
        for c in range(nchunk):
            if c * per >= n:
                assert not r[k][c].any(), f"{what}: the empty chunk {c} of {k} is not all zeros"
            gate(f"{what} {k}[chunk {c}]", r[k][c], ref[k][c], yard[k][c], mult(k), one.get(k, 0.0))
        gate(f"{what} {k} summed", r[k].sum(0), ref[k + "_sum"], yard[k + "_sum"], mult(k), one.get(k, 0.0))
        if case["mask"] is not None:
            dead = ~case["mask"][None, :, None, :, None].expand_as(r[k])
            assert not r[k][dead].any(), f"{what}: {k} is not exactly zero in the rows the mask removes"
    if single.numel():                       # one live row: the VALU kernels take D and dP in one order, dS = 0 exactly
        if not mfma_dq and not d["forms"][0].startswith("fwd<"):
            assert not r["dq"][single].any(), f"{what}: dq of an image with one live row is not exactly zero"
        if not mfma_dkv:
            assert not r["dkf"][:, single].any(), f"{what}: dkf of an image with one live row is not exactly zero"
    if regime == "flat":
        for k, kr in (("out", "out"), ("dq", "dq")):
            old_flat_gate(f"{what} {k}", r[k], ref[kr])
        for k in ("dkf", "dvf"):
            old_flat_gate(f"{what} {k}", r[k].sum(0), ref[k + "_sum"])


@pytest.mark.parametrize("backend", BACKENDS)
def test_folded_attention_rejections(backend):
    """argument checks of mi_folded_attn_fwd / _bwd: the return code, a message, and nothing written.  A pointer that is not 16-byte aligned
    is refused at C = 16 (the matrix-core forms move 16 bytes at a time) -- the refusal is all that is tested, no kernel ever sees one."""
    dev = setup(backend)
    lib = L.lib()
    B, n, H, J = 2, 8, 2, 8
    src = torch.zeros(B * H * 769 * 64 + 4, device=dev)
    flat, buf = guarded((8, B * H * 769 * 64 + 4), torch.float32, dev)
    assert src.data_ptr() % 16 == 0 and buf.data_ptr() % 16 == 0 and (buf[1].data_ptr() % 16 == 0)
    ins, outs = ("q", "kf", "vf", "dout"), ("out", "lse", "dsum", "dq", "dkf", "dvf", "oh")

    def params(**kw):
        p = L.MiFoldedAttnParams()
        p.B, p.n, p.H, p.J, p.C, p.nchunk = B, n, H, J, 16, 1
        for k in ins:
            setattr(p, k, src.data_ptr())
        for i, k in enumerate(outs):
            setattr(p, k, buf[i].data_ptr())
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def refused(fn, code, what, **kw):
        assert lib.mi_layernorm_bwd_nwg(1, 1) == 1 and lib.mi_layernorm_fwd(0, 0, 0, 0, 0, 0, 0, EPS, 0) == MI_ERR_INVALID   # leaves another entry point's message
        assert fn(C.byref(params(**kw)), L.current_stream()) == code, (what, kw)
        msg = lib.mi_last_error().decode()
        assert msg and "mi_folded_attn" in msg, (what, kw, msg)
        return msg
    fwd, bwd = lib.mi_folded_attn_fwd, lib.mi_folded_attn_bwd
    assert fwd(None, L.current_stream()) == MI_ERR_INVALID and bwd(None, L.current_stream()) == MI_ERR_INVALID
    for fn in (fwd, bwd):
        for Cc in (4, 12, 64):
            msg = refused(fn, MI_ERR_UNSUPPORTED, "C", C=Cc)
            assert str(Cc) in msg
        for Cc in (8, 16, 32):
            refused(fn, MI_ERR_UNSUPPORTED, "J * C", C=Cc, J=AT_CAP // Cc + 1)
        for dim in ("B", "n", "H", "J"):
            refused(fn, MI_ERR_INVALID, "size", **{dim: 0})
    for k in ("q", "kf", "vf", "lse", "out"):
        refused(fwd, MI_ERR_INVALID, "NULL", **{k: None})
    for k in ("q", "kf", "vf", "lse", "dout", "dsum", "dq", "dkf", "dvf"):
        refused(bwd, MI_ERR_INVALID, "NULL", **{k: None})
    refused(bwd, MI_ERR_INVALID, "nchunk", nchunk=0)
    for k in ("q", "kf", "vf", "out", "oh"):
        msg = refused(fwd, MI_ERR_INVALID, "alignment", **{k: getattr(params(), k) + 4})
        assert "aligned" in msg
    for k in ("q", "kf", "vf", "dout", "oh", "dq", "dkf", "dvf"):
        msg = refused(bwd, MI_ERR_INVALID, "alignment", **{k: getattr(params(), k) + 4})
        assert "aligned" in msg
    assert torch.isnan(buf).all() and canary_intact(flat.cpu()), "a refused call wrote"
    L.check(fwd(C.byref(params()), L.current_stream()), "mi_folded_attn_fwd, the accepted form of the refused calls")
    L.check(bwd(C.byref(params()), L.current_stream()), "mi_folded_attn_bwd, the accepted form of the refused calls")
    L.check(fwd(C.byref(params(C=8, q=src.data_ptr() + 4)), L.current_stream()), "C = 8 makes no 16-byte access: any float pointer")


@pytest.mark.parametrize("backend", BACKENDS)
def test_train_ops_copy_misaligned_inputs(backend):
    """train_ops never meets the alignment refusals: a contiguous view that starts 4 bytes into a 16-byte line is copied first, and the results
    are those of the aligned tensors, bit for bit"""
    dev = setup(backend)
    g = torch.Generator().manual_seed(5)

    def shifted(t):
        base = torch.zeros(t.numel() + 4, device=dev)
        assert base.data_ptr() % 16 == 0
        v = base[1:1 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        return v
    q, kf, vf, gy = torch.randn(2, 40, 16, generator=g), torch.randn(2, 2, 20, 16, generator=g) * 0.5, torch.randn(2, 2, 20, 16, generator=g), torch.randn(2, 40, 16, generator=g)
    x, w, b, dy = torch.randn(70, 16, generator=g), torch.randn(16, generator=g), torch.randn(16, generator=g), torch.randn(70, 16, generator=g)
    res = []
    train_ops.FORCE = True
    try:
        for prep in (lambda t: t.to(dev), shifted):
            leaves = [prep(t).requires_grad_() for t in (q, kf, vf)]
            gr = torch.autograd.grad(train_ops.folded_attention(*leaves, None), leaves, prep(gy))
            xl, wl, bl = prep(x).requires_grad_(), w.to(dev).requires_grad_(), b.to(dev).requires_grad_()
            assert train_ops.layer_norm_supported(xl, wl)
            y = train_ops.layer_norm(xl, wl, bl, EPS)
            res.append([t.detach().cpu() for t in gr + (y,) + torch.autograd.grad(y, (xl, wl, bl), prep(dy))])
    finally:
        train_ops.FORCE = False
    for a, c in zip(*res):
        assert torch.isfinite(a).all() and torch.equal(bits(a), bits(c))


# ---------------------------------------------------------------------------------------------------------------------------------
# B. LayerNorm

LN_NT, LN_CAP = 256, 512


def ln_launch(rows, dim):
    """(form, rows per workgroup and turn, workgroups, turns per workgroup) of mi_layernorm_bwd: the documented formula of mi_layernorm_bwd_nwg"""
    rows_form = dim in (8, 16, 32)
    per_wg = LN_NT if rows_form else LN_NT // 64
    nwg = min(LN_CAP, -(-rows // per_wg))
    return ("rows" if rows_form else "wave"), per_wg, nwg, -(-rows // (nwg * per_wg))


def ln_forms(rows, dim):
    form, _, nwg, rows_per = ln_launch(rows, dim)
    return (f"ln-{form}/rows_per{rows_per}", "ln-reduce<=256" if nwg <= 256 else "ln-reduce>256")


LN_DIMS = (8, 16, 32, 1, 3, 4, 12, 63, 64, 65, 100, 1023, 1024)
# (rows, dim, data regime)
LN_CASES = ([(rows, dim, "offset30") for dim in LN_DIMS for rows in (1, 255, 256, 257)]
            + [(2051, 12, "offset30"),          # wave form, rows_per = 2: 257 of 512 workgroups hold rows, the others write zero partials
               (1500, 40, "offset30"),          # 256 < nwg = 375 < 512: the strided loop of the reduction
               (131077, 8, "offset30"),         # rows form, rows_per = 2: workgroup 256 holds the last 5 rows, 255 are idle
               (3000, 16, "offset30")]          # rows form, nwg = 12, ragged
            + [(rows, dim, regime) for rows, dim in ((300, 16), (66, 100)) for regime in ("offset1e3", "constrow", "tiny-huge", "dy1e6")])


# (rows, dim, output) where fp32 torch's own F.layer_norm misses err <= 3e-5 max(1, |ref|max) on the offset30 data: rows of 1 .. 4 elements
# around a 30 sigma offset can have next to no variance of their own, and no fp32 evaluation holds 3e-5 there.  The condition does not involve
# the kernel; the test fails when fp32 torch misses the gate anywhere this list does not name.
FLAT_GATE_DROPPED = {(1, 1, 'dgamma'), (255, 1, 'dx'), (255, 1, 'dgamma'), (256, 1, 'dx'), (256, 1, 'dgamma'), (257, 1, 'dx'), (257, 1, 'dgamma'),
                     (256, 3, 'dx'), (257, 3, 'dx')}


@functools.lru_cache(maxsize=None)
def ln_case(rows, dim, regime, with_beta=True):
    g = torch.Generator().manual_seed(rows * 1031 + dim)
    rn = lambda *s: torch.randn(*s, generator=g)
    # (dy around 0.5: dbeta, a plain sum over the rows, is then no cancelled quantity -- at dim 1 it is a tensor of ONE element, and a sum of 255
    # zero-mean terms that lands near zero leaves max |ref| without the scale the yardstick's ulp term needs)
    x, dy, groups = rn(rows, dim) * 2.0 + rn(rows, 1) * 30.0, rn(rows, dim) + 0.5, None
    if regime == "offset1e3":
        x = rn(rows, dim) + 1e3 * (2.0 * torch.randint(0, 2, (rows, 1), generator=g) - 1.0)
    elif regime == "constrow":
        x[rows // 2] = 0.7
    elif regime == "tiny-huge":
        x = rn(rows, dim)
        x[0::2] *= 1e-4
        x[1::2] *= 1e4
        groups = (slice(0, None, 2), slice(1, None, 2))            # dx ~ rstd: the tiny rows' is 1e8 x the huge rows'; each judged on its own
    elif regime == "dy1e6":                 # dx is row-local: judged per group of rows of one magnitude
        dy[0::2] *= 1e-3
        dy[1::2] *= 1e3
        groups = (slice(0, None, 2), slice(1, None, 2))
    gamma, beta = 1.0 + 0.3 * rn(dim), (0.2 * rn(dim) if with_beta else None)
    _, per_wg, nwg, rows_per = ln_launch(rows, dim)
    out = dict(x=x, dy=dy, gamma=gamma, beta=beta, groups=groups)
    for key, dt in (("ref", torch.float64), ("yard", torch.float32)):
        xl, gl = x.to(dt).requires_grad_(), gamma.to(dt).requires_grad_()
        bl = None if beta is None else beta.to(dt).requires_grad_()
        y = F.layer_norm(xl, (dim,), gl, bl, EPS)
        gr = torch.autograd.grad(y, (xl, gl) + (() if bl is None else (bl,)), dy.to(dt))
        xd = xl.detach()
        mean, var = xd.mean(-1), xd.var(-1, unbiased=False)
        rstd = 1.0 / torch.sqrt(var + EPS)
        # the workgroup's share of (dgamma | dbeta): its rows_per turns of per_wg consecutive rows
        terms = torch.stack((dy.to(dt) * (xd - mean[:, None]) * rstd[:, None], dy.to(dt)), 1)               # [rows][2][dim]
        span = per_wg * rows_per
        partial = torch.stack([terms[w * span:(w + 1) * span].sum(0) for w in range(nwg)])
        out[key] = dict(y=y.detach(), stat=torch.stack((mean, rstd), -1), dx=gr[0], dgamma=gr[1], dbeta=gr[2] if bl is not None else None, partial=partial)
    return out


def run_ln(dev, case, rows, dim, stat=True, dgamma=True, dbeta=True, partial=True):
    """mi_layernorm_fwd + mi_layernorm_bwd on guarded buffers -> outputs on the host; the backward always reads a complete stat"""
    lib = L.lib()
    keep = {k: case[k].to(dev).contiguous() for k in ("x", "dy", "gamma", "beta") if case[k] is not None}
    nwg = lib.mi_layernorm_bwd_nwg(rows, dim)
    assert nwg == ln_launch(rows, dim)[2], ("mi_layernorm_bwd_nwg against the documented formula", nwg, ln_launch(rows, dim))
    bufs = {k: guarded(s, torch.float32, dev) for k, s in dict(y=(rows, dim), stat=(rows, 2), dx=(rows, dim), partial=(nwg, 2, dim), dgamma=(dim,), dbeta=(dim,)).items()}
    at = lambda k, on=True: bufs[k][1].data_ptr() if on else 0
    L.check(lib.mi_layernorm_fwd(keep["x"].data_ptr(), keep["gamma"].data_ptr(), L.ptr(keep.get("beta")), at("y"), at("stat", stat), rows, dim, EPS, L.current_stream()),
            "mi_layernorm_fwd")
    if not stat:                            # the backward needs one: a second forward, which must give the same y
        y1 = bufs["y"][1].cpu().clone()
        L.check(lib.mi_layernorm_fwd(keep["x"].data_ptr(), keep["gamma"].data_ptr(), L.ptr(keep.get("beta")), at("y"), at("stat"), rows, dim, EPS, L.current_stream()),
                "mi_layernorm_fwd")
        assert torch.isnan(y1).sum() == 0 and torch.equal(bits(y1), bits(bufs["y"][1].cpu())), "stat = NULL changes y"
    L.check(lib.mi_layernorm_bwd(keep["dy"].data_ptr(), keep["x"].data_ptr(), keep["gamma"].data_ptr(), at("stat"), at("dx"), at("partial", partial), at("dgamma", dgamma),
                                 at("dbeta", dbeta), rows, dim, L.current_stream()), "mi_layernorm_bwd")
    res = {}
    for k, (flat, view) in bufs.items():
        flat, res[k] = host(flat, view)
        assert canary_intact(flat), f"the elements after {k} were overwritten"
    for k in keep:
        assert torch.equal(bits(keep[k].cpu()), bits(case[k])), f"the input {k} was written"
    return res


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", LN_CASES, ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}")
def test_layernorm_direct(backend, case):
    """mi_layernorm_fwd + mi_layernorm_bwd against F.layer_norm and its autograd in fp64: y, the saved (mean, rstd) against the fp64 mean and
    1 / sqrt(var + eps), dx, dgamma, dbeta, and every workgroup's row of `partial` against the fp64 sums over that workgroup's rows (idle
    workgroups: exact zeros), each within the fp32 yardstick.  dy1e6: dx per group of rows of one magnitude."""
    rows, dim, regime = case
    dev = setup(backend)
    what = f"layernorm {backend} {rows}x{dim} {regime} {ln_forms(rows, dim)}"
    c = ln_case(rows, dim, regime)
    ref, yard = c["ref"], c["yard"]
    runs = [run_ln(dev, c, rows, dim) for _ in range(2)]
    for k in runs[0]:
        assert torch.equal(bits(runs[0][k]), bits(runs[1][k])), f"{what}: {k} differs between two runs"
    r = runs[0]
    for k in ("y", "dgamma", "dbeta", "partial"):
        within_yardstick(f"{what} {k}", r[k], ref[k], yard[k])
    for i, k in enumerate(("mean", "rstd")):
        within_yardstick(f"{what} {k}", r["stat"][:, i], ref["stat"][:, i], yard["stat"][:, i])
    for sl in c["groups"] or (slice(None),):
        within_yardstick(f"{what} dx[{sl.start}::{sl.step}]", r["dx"][sl], ref["dx"][sl], yard["dx"][sl])
    _, per_wg, nwg, rows_per = ln_launch(rows, dim)
    idle = -(-rows // (per_wg * rows_per))
    assert not r["partial"][idle:].any(), f"{what}: the {nwg - idle} idle workgroups do not write zero partials"
    if regime == "offset30":                 # the gate of test_training, except where the same formula in fp32 torch ops misses it itself: FLAT_GATE_DROPPED
        for k in ("y", "dx", "dgamma", "dbeta"):
            torch_meets = (yard[k].double() - ref[k]).abs().max().item() <= FLAT_GATE * max(1.0, ref[k].abs().max().item())
            assert torch_meets or (rows, dim, k) in FLAT_GATE_DROPPED, (what, k, "fp32 torch misses the 3e-5 gate at a case FLAT_GATE_DROPPED does not list")
            if torch_meets:
                old_flat_gate(f"{what} {k}", r[k], ref[k])


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("shape", [(300, 16), (66, 100), (2051, 12)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_layernorm_optional_arguments(backend, shape):
    """stat = NULL, beta = NULL, dgamma = NULL with partial = NULL (dx only), dbeta = NULL with dgamma given: what is still produced is bit-equal
    to the full call, what is not asked for stays untouched"""
    rows, dim = shape
    dev = setup(backend)
    c = ln_case(rows, dim, "offset30")
    full = run_ln(dev, c, rows, dim)
    eq = lambda a, b, k: torch.isfinite(a[k]).all() and torch.equal(bits(a[k]), bits(b[k]))
    r = run_ln(dev, c, rows, dim, stat=False)
    assert all(eq(r, full, k) for k in full), "stat = NULL"
    r = run_ln(dev, c, rows, dim, dgamma=False, dbeta=False, partial=False)
    assert eq(r, full, "dx") and all(torch.isnan(r[k]).all() for k in ("partial", "dgamma", "dbeta")), "dgamma = NULL: dx only"
    r = run_ln(dev, c, rows, dim, dgamma=False, dbeta=False)
    assert eq(r, full, "dx") and all(torch.isnan(r[k]).all() for k in ("partial", "dgamma", "dbeta")), "dgamma = NULL with a workspace: dx only"
    r = run_ln(dev, c, rows, dim, dbeta=False)
    assert all(eq(r, full, k) for k in ("dx", "partial", "dgamma")) and torch.isnan(r["dbeta"]).all(), "dbeta = NULL"
    nb = ln_case(rows, dim, "offset30", False)
    r = run_ln(dev, nb, rows, dim, dbeta=False)
    within_yardstick(f"layernorm {backend} {rows}x{dim} beta = NULL: y", r["y"], nb["ref"]["y"], nb["yard"]["y"])
    assert all(eq(r, full, k) for k in ("stat", "dx", "partial", "dgamma")), "beta = NULL changes more than y"


@pytest.mark.parametrize("backend", BACKENDS)
def test_layernorm_rejections(backend):
    """argument checks of mi_layernorm_fwd / _bwd / _bwd_nwg: the return code, a message, nothing written; pointers that are not 16-byte aligned are
    refused at dim 8 / 16 / 32 (refusal only: no kernel sees one) and accepted by the wave form"""
    dev = setup(backend)
    lib = L.lib()
    rows, dim = 8, 16
    src = torch.ones(rows * 1025 + 4, device=dev)
    flat, buf = guarded((6, rows * 1025 + 4), torch.float32, dev)
    assert src.data_ptr() % 16 == 0 and buf.data_ptr() % 16 == 0 and buf[1].data_ptr() % 16 == 0
    s, (y, stat, dx, partial, dgamma, dbeta) = src.data_ptr(), [buf[i].data_ptr() for i in range(6)]
    st = L.current_stream()

    def refused(rc, what):
        assert rc == MI_ERR_INVALID, what                               # (the message checked below is this call's: every call here is refused)
        msg = lib.mi_last_error().decode()
        assert msg and "mi_layernorm" in msg, (what, msg)
        return msg
    for r, d in ((0, dim), (-3, dim), (rows, 0), (rows, 1025)):
        refused(lib.mi_layernorm_fwd(s, s, s, y, stat, r, d, EPS, st), ("fwd", r, d))
        refused(lib.mi_layernorm_bwd(s, s, s, s, dx, partial, dgamma, dbeta, r, d, st), ("bwd", r, d))
        assert lib.mi_layernorm_bwd_nwg(r, d) == 0
    for args in ((0, s, s, y, stat), (s, 0, s, y, stat), (s, s, s, 0, stat)):
        refused(lib.mi_layernorm_fwd(*args, rows, dim, EPS, st), "fwd NULL")
    for args in ((0, s, s, s, dx), (s, 0, s, s, dx), (s, s, 0, s, dx), (s, s, s, 0, dx), (s, s, s, s, 0)):
        refused(lib.mi_layernorm_bwd(*args, partial, dgamma, dbeta, rows, dim, st), "bwd NULL")
    refused(lib.mi_layernorm_bwd(s, s, s, s, dx, 0, dgamma, dbeta, rows, dim, st), "dgamma without partial")
    for d in (8, 16, 32):
        for args in ((s + 4, s, s, y, stat), (s, s, s, y + 4, stat), (s, s, s, y, stat + 4)):
            assert "aligned" in refused(lib.mi_layernorm_fwd(*args, rows, d, EPS, st), "fwd alignment")
        for args in ((s + 4, s, s, s, dx), (s, s + 4, s, s, dx), (s, s, s, s + 4, dx), (s, s, s, s, dx + 4)):
            assert "aligned" in refused(lib.mi_layernorm_bwd(*args, partial, dgamma, dbeta, rows, d, st), "bwd alignment")
    assert torch.isnan(buf).all() and canary_intact(flat.cpu()), "a refused call wrote"
    L.check(lib.mi_layernorm_fwd(s, s, s, y, stat, rows, dim, EPS, st), "the accepted form of the refused calls")
    L.check(lib.mi_layernorm_bwd(s, s, s, stat, dx, partial, dgamma, dbeta, rows, dim, st), "the accepted form of the refused calls")
    L.check(lib.mi_layernorm_fwd(s + 4, s, s, y + 4, stat, rows, 12, EPS, st), "the wave form reads single floats: any float pointer")
    L.check(lib.mi_layernorm_bwd(s + 4, s + 4, s, stat, dx + 4, partial, dgamma, dbeta, rows, 12, st), "the wave form reads single floats: any float pointer")


# ---------------------------------------------------------------------------------------------------------------------------------

REQUIRED_FORMS = ({f"{k}<{tw}>/{njt}" for k in ("fwd", "dq") for tw in ("1,4", "2,4", "2,8") for njt in (17, 24)}
                  | {"dkv<12,4>", "dkv<18,6>", "dkv<24,8>"} | {f"{k}-valu{c}" for k in ("fwd", "dq", "dkv") for c in (8, 16, 32)} | {"dq+oh", "dq-oh"}
                  | {f"ln-{f}/rows_per{r}" for f in ("rows", "wave") for r in (1, 2)} | {"ln-reduce<=256", "ln-reduce>256"})


def test_every_launch_form_is_reached():
    """every instantiation the two dispatches can pick is reached by at least one fp64-judged case above -- computed from the dispatch rules as
    restated in attn_forms / ln_forms, not from the cases' labels; on the GPU no case is skipped, the emulator skips EMU_SLOW"""
    reached = set()
    for d in ATTN_CASES:
        reached |= set(attn_forms(d["B"], d["n"], d["H"], d["J"], d["C"], d["valu"], d["oh"]))
    for rows, dim, _ in LN_CASES:
        reached |= set(ln_forms(rows, dim))
    assert not REQUIRED_FORMS - reached, sorted(REQUIRED_FORMS - reached)
