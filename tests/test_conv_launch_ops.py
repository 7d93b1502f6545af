"""Op-level fp64 parity of the forward conv family (csrc/conv.hip, conv_rp.hip, conv_stripe.hip, conv_wide.hip with mi_gn_coef_fwd and
mi_conv_prep_fwd) launched THE WAY THE ENGINE LAUNCHES IT (engine.py / conv_route.py; the recorded plans in tests/golden/conv_plans.txt.gz),
which the arithmetic tests of test_kernels.py / test_conv_stripe.py do not do:

A  input statistics arrive as SEVERAL tiles (mi_act.nt > 1) of unequal size on every consumer path: mi_gn_channel_totals' unrolled and tail
   loops and its passes, the register fast paths mi_gn_totals_issue / st_totals_issue with their nt limit and their fallbacks, the residual
   side, the direct family's reads, mi_gn_coef_fwd;
B  rows shared between the two guidance halves (mi_act.bmod) on in0 / res0 / in1 / res1, data and statistics;
C  the engine's flag words on the direct family (MI_CONV_SPLIT16 | MI_CONV_SPLIT8) at the sizes of the 20 x 20 plan: every dispatch branch of
   mi_conv_fwd's direct part, flagged against unflagged bit for bit;
D  the placement-only parts of the tile_cfg word (MI_CONV_REVERSE, strip counts, the split flags on the matrix-core families) leave the bits
   alone, the exact words of the recorded plans included; every recorded word is launched by a case of this file;
E  statistics hand-offs between two launches of different kernel families (out_stats / out_nt of one conv as the next one's mi_act.stats / nt),
   and conv 1's out_stats per tile.

Every reference is fp64 torch on the CPU.  Gates are the family's own: err < 2e-5 * max(1, max |ref| / 8) (test_conv_row_paired_path) for the
three-term kernels behind a GroupNorm, conv_gate_per_image for the plain convs (images of different magnitude), 2e-3 max |ref| + 2^-8 |ref| for
the single-term bf16 form (test_conv_row_paired_bf16_storage); the ratio against fp32 torch on the CPU is printed, not gated.

Inputs make a misread visible: image b and channel c have their own magnitude (factors 2.5 apart) and offset, the statistics tiles are cut at
random unequal places, every statistics buffer is followed by at least 128 fp64 entries of 1e30, and a tensor shared through bmod holds only
bmod rows: the rows b >= bmod of the allocation hold 1e30 (finite values in valid memory) in data and statistics.  Outputs are pre-filled with
NaN and followed by a canary, every launch of A, B, C and E runs twice and must repeat its bits."""
import ctypes as C
import functools
import gzip
import os
import re
from typing import NamedTuple

import pytest
import torch
import torch.nn.functional as F

from minimagen_amd import _lib as L, packing as P
from tests._backend import BACKENDS, setup
from tests.test_block_bwd_ops import bits, canary_intact, conv_gate_per_image, group_act, guarded, piece_stats, ss_table, unequal_cuts
from tests.test_kernels import check_stats, tile_nt

SK = 2 ** -0.5
POISON = 1e30
POISON_TAIL = 2 * 64                                       # fp64 entries of POISON behind every statistics buffer
MAGS = [2.5 ** k for k in (0, 1, -1, 2, -2, 3, -3, 4)]     # per-image magnitude of the conv inputs
RES_MAGS = [1.0, 2.0, 0.5, 4.0, 0.25, 3.0, 0.75, 1.5]      # ... of the residual inputs (they reach the output unnormalised: kept near 1 so the gate stays tight)
SS_PAD, SS_OFF = 7, 7                                      # scale / shift table: ss_stride = 2 Cin + 7, ss_off = 7
SPLIT16, REVERSE, HALF, SPLIT8 = 0x100, 0x200, 0x400, 0x800
ENGINE = SPLIT16 | SPLIT8                                  # what conv_route.tile_word puts on every small launch
PLANS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plans.txt.gz")


class Case(NamedTuple):
    """one launch: tile code, batch, channels of in0 + in1 -> Cout, OUTPUT size, statistics tiles of (in0, in1, res0, res1)"""
    name: str
    code: int
    B: int
    C0: int
    C1: int
    Cout: int
    H: int
    W: int
    nt: tuple = (1, 1, 1, 1)
    mode: str = "k3"                # "k3" | "up2" (nearest x2 + k3) | "k4s2"
    gn: bool = True                 # GroupNorm(8) -> scale / shift -> SiLU in front; False: plain conv with in0.stats given (the rms scaling)
    res: object = "none"            # "none" | "id" | (Cres0, Cres1): 1x1 conv over their concat
    bmod: tuple = (0, 0, 0, 0)      # mi_act.bmod of (in0, in1, res0, res1)
    half: bool = False              # single-term kernels (tile_cfg | 0x400) on bf16 storage
    wide: bool = False              # wide regime of conv_rp.hip (gn_coef / gn_exps from mi_gn_coef_fwd); tile code 11 implies it
    flags: int = 0                  # further bits of the tile_cfg word

    @property
    def family(self):
        return "direct" if self.code <= 2 else "stripe" if self.code == 12 else "gemm" if self.code == 11 else "wide" if self.wide else "narrow"

    @property
    def word(self):
        return self.code | (HALF if self.half else 0) | self.flags

    def __str__(self):
        return self.name


def expand(t, B, bm):
    """the B rows a kernel sees of a tensor that holds bm rows (row b -> b % bm)"""
    return t if not bm else t[torch.arange(B) % bm]


def tensors_of(c: Case):
    """the host tensors of a case: inputs with their own magnitude per image and offset per channel, their statistics in unequal tiles"""
    g = torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(c.name)) & 0xffffff)
    rn = lambda *s: torch.randn(*s, generator=g)
    ks, stride = (4, 2) if c.mode == "k4s2" else (3, 1)
    Hin, Win = (c.H // 2, c.W // 2) if c.mode == "up2" else (c.H * stride, c.W * stride)
    Cin = c.C0 + c.C1
    st16 = (lambda t: t.bfloat16()) if c.half else (lambda t: t)
    t = dict(Hin=Hin, Win=Win, ks=ks, stride=stride)

    def act(key, Cc, bm, n, nt, mags, off):
        R = bm or c.B
        x = torch.randn(R, Cc, n, generator=g)
        u = (0.5 + 0.5 * torch.rand(Cc, generator=g)) * (2.0 * torch.randint(0, 2, (Cc,), generator=g) - 1.0)      # offsets of either sign (offset_input)
        x = st16(1.5 * (x + off * u[None, :, None]) * torch.tensor(mags[:R])[:, None, None])
        t[key] = x
        t[key + "_stats"] = piece_stats(x.float(), unequal_cuts(n, nt, g))

    act("x0", c.C0, c.bmod[0], Hin * Win, c.nt[0], MAGS, 3.0)
    if c.C1:
        act("x1", c.C1, c.bmod[1], Hin * Win, c.nt[1], MAGS[::-1], 3.0)
    wsc = 0.2 if Cin <= 32 else 0.5 / (Cin * ks * ks) ** 0.5
    t["w"], t["bias"] = rn(c.Cout, Cin, ks, ks) * wsc, rn(c.Cout)
    if c.gn:
        t["gamma"], t["beta"] = 1 + 0.3 * rn(Cin), 0.2 * rn(Cin)
        t["scale"], t["shift"] = 0.3 * rn(c.B, Cin), 0.3 * rn(c.B, Cin)          # one row per image, never shared: rows b and b + bmod differ
    if c.res == "id":
        act("r0", c.Cout, c.bmod[2], c.H * c.W, c.nt[2], RES_MAGS, 0.5)
    elif c.res != "none":
        cr0, cr1 = c.res
        act("r0", cr0, c.bmod[2], c.H * c.W, c.nt[2], RES_MAGS, 0.5)
        if cr1:
            act("r1", cr1, c.bmod[3], c.H * c.W, c.nt[3], RES_MAGS[::-1], 0.5)
        t["rw"], t["rb"] = rn(c.Cout, cr0 + cr1, 1, 1) * (0.3 if cr0 + cr1 <= 32 else 0.1), rn(c.Cout)
    return t


def reference(c: Case, t, dt):
    """the conv of include/minimagen_hip.h in torch ops of dtype dt on the CPU, the shared rows expanded"""
    cast = lambda v: v.to(dt)
    x = expand(cast(t["x0"]), c.B, c.bmod[0])
    if c.C1:
        x = torch.cat((x, expand(cast(t["x1"]), c.B, c.bmod[1]) * SK), 1)
    if c.gn:
        x = group_act(x, cast(t["gamma"]), cast(t["beta"]), cast(t["scale"]), cast(t["shift"]), 8)
    x = x.reshape(c.B, c.C0 + c.C1, t["Hin"], t["Win"])
    if c.mode == "up2":
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    y = F.conv2d(x, cast(t["w"]), cast(t["bias"]), stride=t["stride"], padding=1)
    if c.res == "id":
        y = y + expand(cast(t["r0"]), c.B, c.bmod[2]).reshape(y.shape)
    elif c.res != "none":
        r = expand(cast(t["r0"]), c.B, c.bmod[2])
        if c.res[1]:
            r = torch.cat((r, expand(cast(t["r1"]), c.B, c.bmod[3]) * SK), 1)
        y = y + F.conv2d(r.reshape(c.B, -1, c.H, c.W), cast(t["rw"]), cast(t["rb"]))
    return y


@functools.lru_cache(maxsize=None)
def host_case(c: Case):
    """tensors, fp64 reference and fp32 yardstick of a case, computed once and shared by both backends and every word it is launched with"""
    t = tensors_of(c)
    t["ref"], t["yard"] = reference(c, t, torch.float64), reference(c, t, torch.float32)
    return t


class Prepared:
    """the device copies of a case's tensors and its parameter struct without tile_cfg / out / out_stats"""

    def __init__(self, dev, c: Case, t):
        self.dev, self.c, self.keep = dev, c, {}
        lib = L.lib()
        d = lambda name, v: self.keep.setdefault(name, v.to(dev).contiguous())
        st = 1 if c.half else 0
        fam = c.family

        def view(key, Cc, bm, nt, scale, with_stats=True):
            """mi_act over `key`: the allocation has c.B rows, the tensor bm of them -- the rest, and the tail of the statistics, is POISON"""
            x, s = t[key], t[key + "_stats"]
            missing = c.B - x.shape[0]
            xd = d(key, torch.cat((x.reshape(-1), torch.full((missing * x[0].numel(),), POISON, dtype=x.dtype))))
            sp = 0
            if with_stats:
                sp = d(key + "_stats", torch.cat((s.reshape(-1), torch.full((max(POISON_TAIL, missing * s[0].numel()),), POISON, dtype=torch.float64)))).data_ptr()
            return L.MiAct(xd.data_ptr(), Cc, sp, nt if with_stats else 0, scale, bm, st)

        p = self.p = L.MiConvParams()
        p.B, p.H, p.W = c.B, c.H, c.W
        p.in0 = view("x0", c.C0, c.bmod[0], c.nt[0], 1.0)
        if c.C1:
            p.in1 = view("x1", c.C1, c.bmod[1], c.nt[1], SK)
        Cin = c.C0 + c.C1
        p.Cout, p.ksize, p.stride, p.up2 = c.Cout, t["ks"], t["stride"], int(c.mode == "up2")
        pack = P.pack_conv_weight_ig if fam == "gemm" else P.pack_conv_weight_rp
        ct = lib.mi_conv_cout_tile(c.Cout)
        if fam == "direct":
            p.w = d("w", P.pack_conv_weight(t["w"], ct)).data_ptr()
        else:
            wf, p.w_rp_exp = pack(t["w"])
            p.w_rp = d("wf", wf).data_ptr()
        p.bias = d("bias", t["bias"]).data_ptr()
        if c.gn:
            p.gn_groups, p.gn_gamma, p.gn_beta, p.gn_eps = 8, d("gamma", t["gamma"]).data_ptr(), d("beta", t["beta"]).data_ptr(), 1e-5
            p.scale_shift = d("ss", ss_table(c.B, Cin, t["scale"], t["shift"], 2 * Cin + SS_PAD, SS_OFF)).data_ptr()
            p.ss_stride, p.ss_off = 2 * Cin + SS_PAD, SS_OFF
        self.cres = 0
        if c.res != "none":
            # (the direct family multiplies in fp32 and reads no statistics of its residual)
            p.res0 = view("r0", t["r0"].shape[1], c.bmod[2], c.nt[2], 1.0, with_stats=fam != "direct")
            if c.res != "id":
                self.cres = sum(c.res)
                if c.res[1]:
                    p.res1 = view("r1", c.res[1], c.bmod[3], c.nt[3], SK, with_stats=fam != "direct")
                if fam == "direct":
                    p.res_w = d("rw", P.pack_conv_weight(t["rw"], ct).reshape(self.cres, -1)).data_ptr()
                else:
                    p.res_w = 1                                 # non-null marker: the residual is a 1x1 conv
                    rwf, p.res_w_rp_exp = pack(t["rw"])
                    p.res_w_rp = d("rwf", rwf).data_ptr()
                p.res_b = d("rb", t["rb"]).data_ptr()
        p.out_st = st
        if fam == "stripe":
            rows = lib.mi_conv_stripe_rows(C.byref(p))
            assert rows == c.W // 8, f"{c}: the stripe kernel does not take this launch"
            self.out_nt = c.H // rows
            self.tile = (rows, c.W)
        else:
            th, tw = C.c_int(), C.c_int()
            lib.mi_conv_tile_shape(c.code, C.byref(th), C.byref(tw))
            self.out_nt = tile_nt(lib, c.code, c.H, c.W)
            self.tile = (th.value, tw.value)

    def run(self, word, check=True):
        """one launch with tile_cfg = word on fresh guarded buffers -> (out, out_stats) on the device (views of the guarded buffers)"""
        c, p, dev, lib = self.c, self.p, self.dev, L.lib()
        bufs = dict(out=guarded((c.B, c.Cout, c.H, c.W), torch.bfloat16 if c.half else torch.float32, dev),
                    out_stats=guarded((c.B, c.Cout, self.out_nt, 2), torch.float64, dev))
        if c.family in ("wide", "gemm"):
            bufs["gn_coef"] = guarded((c.B, c.C0 + c.C1, 4), torch.float32, dev)
            bufs["gn_exps"] = guarded((c.B, 2), torch.int32, dev)
        if c.family == "gemm":
            p.act_prep_bytes = lib.mi_conv_prep_bytes(c.B, c.C0 + c.C1, self.cres, c.H, c.W)
            bufs["act_prep"] = guarded((p.act_prep_bytes // 4,), torch.float32, dev)
        for k, (_, v) in bufs.items():
            setattr(p, k, v.data_ptr())
        p.tile_cfg = word
        if "gn_coef" in bufs:
            L.check(lib.mi_gn_coef_fwd(C.byref(p), L.current_stream()), f"{c}: mi_gn_coef_fwd")
        if "act_prep" in bufs:
            L.check(lib.mi_conv_prep_fwd(C.byref(p), L.current_stream()), f"{c}: mi_conv_prep_fwd")
        L.check(lib.mi_conv_fwd(C.byref(p), L.current_stream()), f"{c}: mi_conv_fwd with tile_cfg {word:#x}")
        if check:
            for k, (flat, _) in bufs.items():
                assert canary_intact(flat.cpu()), f"{c} {word:#x}: the elements after {k} were overwritten"
        self.last = bufs
        return bufs["out"][1], bufs["out_stats"][1]


def gate(what, c: Case, out, ost, ref, yard):
    """the family's gate on the output, check_stats' totals on out_stats; prints error / gate and fp32 torch / gate; -> error / gate"""
    out, ost = out.cpu(), ost.cpu()
    assert torch.isfinite(out).all() and torch.isfinite(ost).all(), f"{what}: output or statistics not finite / not fully written"
    err = (out.double() - ref).abs()
    yerr = (yard.double() - ref).abs()
    refmax = ref.abs().max().item()
    if c.half:                          # single fp16 term per product + bf16 rounding of the stored result, per element
        tol = 2e-3 * refmax + 2.0 ** -8 * ref.abs()
        ratio, yratio = (err / tol).max().item(), (yerr / tol).max().item()
    elif not c.gn:                      # plain conv: every image is held to its own magnitude (asserts inside)
        ratio = max(conv_gate_per_image(what, out.float(), ref, yard)) / 2e-5
        yratio = max((yerr[b].max() / ref[b].abs().max()).item() for b in range(c.B)) / 2e-5
    else:
        tol = 2e-5 * max(1.0, refmax / 8.0)
        ratio, yratio = err.max().item() / tol, yerr.max().item() / tol
    print(f"{what}: max|d| {err.max().item():.2e}, |ref|max {refmax:.3g}, error / gate {ratio:.3f}, fp32 torch / gate {yratio:.3f}")
    assert ratio < 1.0, (what, ratio)
    check_stats(ost, ref.float(), rtol=2e-3 if c.half else 1e-5)
    return ratio


def rows_differ(what, c: Case, out):
    """rows b and b + bmod share in0 (or res0) but not scale / shift: a kernel that folds them must not pass"""
    bm = next(m for m in c.bmod if m)
    out = out.cpu()
    for b in range(c.B - bm):
        assert not torch.equal(out[b], out[b + bm]), f"{what}: images {b} and {b + bm} came out equal"


def run_case(backend, c: Case, words=()):
    """the case at its own word, twice with equal bits, against fp64; then once at each of `words`, bit for bit equal to the first"""
    dev = setup(backend)
    t = host_case(c)
    prep = Prepared(dev, c, t)
    what = f"{c} [{backend} {c.family} {c.word:#x}]"
    out, ost = prep.run(c.word)
    out2, ost2 = prep.run(c.word)
    assert torch.equal(bits(out.float()), bits(out2.float())) and torch.equal(bits(ost), bits(ost2)), f"{what}: two runs differ"
    ratio = gate(what, c, out, ost, t["ref"], t["yard"])
    if any(c.bmod):
        rows_differ(what, c, out)
    for w in words:
        o, s = prep.run(w)
        assert torch.equal(bits(o.float()), bits(out.float())), f"{what}: tile_cfg {w:#x} changes the output, max|d| {(o.float() - out.float()).abs().max().item():.3e}"
        assert torch.equal(bits(s), bits(ost)), f"{what}: tile_cfg {w:#x} changes the statistics"
    return ratio


# ---------------------------------------------------------------------------------------------------------------------------------
# A. multi-tile statistics on every consumer path.  TPC = lanes per channel of the totals (common.hip.h: doubled from 1 while TPC < 64 and
#    2 TPC Cin <= nlanes, i.e. the largest power of two <= 64 with TPC Cin <= nlanes); the register fast paths take nt <= MI_STATS_K TPC = 8 TPC.

MULTI_TILE_CASES = [
    # row-paired 8 x 64, 256 lanes, Cin 8: TPC 32, fast path up to nt 256
    Case("rp6-nt5", 6, 2, 8, 0, 8, 16, 64, (5, 1, 1, 1)),                                  # fast path, slot 0 of lanes sub < 5 only: ragged
    Case("rp6-nt40", 6, 2, 8, 0, 8, 16, 64, (40, 1, 1, 1)),                                # ... slot 0 of every lane, slot 1 of lanes sub < 8
    Case("rp6-nt256", 6, 2, 8, 0, 8, 16, 64, (256, 1, 1, 1)),                              # the last nt on the fast path: every slot of every lane
    Case("rp6-nt257", 6, 2, 8, 0, 8, 16, 64, (257, 1, 1, 1)),                              # the first on the fallback: unrolled loop twice, and a tail tile for sub 0
    # row-paired 8 x 32, Cin 24: TPC 8, fast path up to nt 64
    Case("rp7-16+8-nt4/16", 7, 2, 16, 8, 16, 16, 32, (4, 16, 1, 1)),                       # in1.nt > in0.nt: nt_max = in1.nt, fast path
    Case("rp7-16+8-nt4/70", 7, 2, 16, 8, 16, 16, 32, (4, 70, 1, 1)),                       # in0 fits the registers, in1 does not: nt_max sends both to the fallback
    # Cin = 64 = RP_MAXC: TPC 4, fast path up to 32 -> fallback; in1 (nt 33) runs the unrolled loop twice + a tail tile for sub 0, in0 (nt 7) the tail only
    Case("rp7-48+16-nt7/33", 7, 1, 48, 16, 16, 8, 32, (7, 33, 1, 1)),
    # 1x1 residual over a concat of 24: TPC 8; its statistics set the residual operand's exponent (res_stats): fast2, and its fallback
    Case("rp7-res8+16-nt3/20", 7, 1, 16, 0, 16, 16, 32, (2, 1, 3, 20), res=(8, 16)),
    Case("rp7-res8+16-nt3/70", 7, 1, 16, 0, 16, 16, 32, (2, 1, 3, 70), res=(8, 16)),
    # stripe kernel at 64 wide: 256 lanes of MFMA waves, Cin 16: TPC 16, st_totals_issue covers nt <= 128; 130 -> the fallback behind it (mi_gn_channel_totals)
    Case("stripe-8+8-nt130/3", 12, 2, 8, 8, 8, 16, 64, (130, 3, 1, 1)),
    Case("stripe-8+8-nt3/130", 12, 2, 8, 8, 8, 16, 64, (3, 130, 1, 1)),                    # ... by in1.nt alone (its nt_max)
    Case("stripe-8+8-nt5/3", 12, 2, 8, 8, 8, 16, 64, (5, 3, 1, 1)),                        # ... and covered
    Case("stripe-res8+8-nt8,4/9", 12, 1, 8, 0, 8, 16, 64, (8, 1, 4, 9), res=(8, 8)),       # the residual loader wave's totals: 64 lanes, Cres 16: TPC 4, covered up to 32
    Case("stripe-res8+8-nt8,4/40", 12, 1, 8, 0, 8, 16, 64, (8, 1, 4, 40), res=(8, 8)),     # ... their fallback
    Case("stripe-up2-nt3", 12, 1, 16, 0, 8, 16, 64, (3, 1, 1, 1), mode="up2", gn=False),   # plain convs: operand scaling from multi-tile statistics
    Case("stripe-k4s2-nt3", 12, 1, 8, 0, 8, 8, 64, (3, 1, 1, 1), mode="k4s2", gn=False),
    Case("stripe-plain-nt3", 12, 1, 8, 0, 8, 16, 64, (3, 1, 1, 1), gn=False),
    # direct family: tile 2 has 64 lanes, Cin 64: TPC 1, one pass, in0 (nt 70) runs the unrolled loop 17 x + 2 tail tiles
    Case("direct2-40+24-nt70/9", 2, 2, 40, 24, 16, 8, 32, (70, 9, 1, 1)),
    Case("direct0-nt200", 0, 1, 8, 0, 8, 16, 64, (200, 1, 1, 1)),                          # 256 lanes, Cin 8: TPC 32, unrolled loop once (four tiles in flight) + 2 .. 3 tail tiles
    Case("direct2-plain-nt3", 2, 1, 8, 0, 8, 8, 32, (3, 1, 1, 1), gn=False),
    # wide regime: mi_gn_coef_fwd (256 lanes).  Cin 160: TPC 1, ONE pass of 256 channels; Cin 288: TPC 1, TWO passes (channels 256 .. 287 in the second)
    Case("wide7-96+64-nt5/12,3/7", 7, 1, 96, 64, 72, 8, 32, (5, 12, 3, 7), res=(96, 64), wide=True),
    Case("wide7-288-nt6", 7, 1, 288, 0, 32, 8, 32, (6, 1, 1, 1), wide=True),
    Case("wide7-plain-nt5", 7, 1, 64, 0, 32, 8, 32, (5, 1, 1, 1), gn=False, wide=True),
    Case("wide10-nt3", 10, 1, 32, 0, 32, 16, 16, (3, 1, 1, 1), wide=True),
    Case("gemm11-nt6", 11, 1, 64, 0, 128, 8, 16, (6, 1, 1, 1)),                            # mi_gn_coef_fwd + mi_conv_prep_fwd; Cin 64: TPC 4, tail loop only
    Case("gemm11-plain-nt4", 11, 1, 64, 0, 64, 8, 16, (4, 1, 1, 1), gn=False),
    # the up / down-sampling members of the tile kernel (plain convs)
    Case("rp6-up2-nt3", 6, 1, 16, 0, 8, 16, 64, (3, 1, 1, 1), mode="up2", gn=False),
    Case("rp7-k4s2-nt3", 7, 1, 8, 0, 16, 8, 32, (3, 1, 1, 1), mode="k4s2", gn=False),
    Case("rp7-plain-nt5", 7, 1, 8, 0, 8, 16, 32, (5, 1, 1, 1), gn=False),
    # the HALF instantiation of the same prologue, activations stored as bf16
    Case("half7-8+8-nt5/2", 7, 2, 8, 8, 8, 16, 32, (5, 2, 1, 1), half=True),
]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", MULTI_TILE_CASES, ids=str)
def test_multi_tile_statistics(backend, case):
    """A: the conv with its inputs' statistics in nt > 1 unequal tiles against fp64 (the consumers only add partials: any partition of the
    pixels is a legal producer layout).  A tile read past nt meets the next channel's record or 1e30, a dropped tile moves the moments of a
    channel whose offset is 1.5 .. 3 sigma: both far outside the gate."""
    run_case(backend, case)


# ---------------------------------------------------------------------------------------------------------------------------------
# B. rows shared between the guidance halves

BMOD_FAMILIES = [
    # name, code, C0, Cout, H, W, extra
    ("rp6", 6, 8, 8, 16, 64, {}),
    ("rp7", 7, 16, 16, 8, 32, {}),
    ("stripe", 12, 8, 8, 16, 64, {}),
    ("direct2", 2, 8, 8, 8, 32, {}),
    ("wide7", 7, 32, 32, 8, 32, dict(wide=True)),
    ("wide10", 10, 32, 32, 16, 16, dict(wide=True)),
    ("gemm11", 11, 32, 64, 8, 16, {}),                     # identity residual of conv_wide.hip
    ("half7", 7, 8, 8, 16, 32, dict(half=True)),
]
BMOD_CASES = [Case(f"bmod-{name}-B{B}m{bm}-{which}", code, B, C0, 0, Cout, H, W, (3, 1, 2, 1), res="id",
                   bmod=(bm if which != "res0" else 0, 0, bm if which != "in0" else 0, 0), **extra)
              for name, code, C0, Cout, H, W, extra in BMOD_FAMILIES
              for B, bm in ((4, 2), (2, 1), (8, 4))                    # B = 8 also takes the XCD-aware workgroup -> image map
              for which in ("both", "in0", "res0")]
BMOD_CASES += [
    Case("bmod-rp7-in0-not-in1", 7, 4, 16, 8, 16, 16, 32, (3, 5, 1, 1), bmod=(2, 0, 0, 0)),
    Case("bmod-rp7-in1-not-in0", 7, 4, 16, 8, 16, 16, 32, (3, 5, 1, 1), bmod=(0, 2, 0, 0)),
    Case("bmod-rp7-res0-not-res1", 7, 4, 16, 0, 16, 16, 32, (2, 1, 3, 5), res=(8, 16), bmod=(0, 0, 2, 0)),
    Case("bmod-stripe-res0-not-res1", 12, 4, 8, 0, 8, 16, 64, (2, 1, 3, 5), res=(8, 8), bmod=(0, 0, 2, 0)),
    Case("bmod-direct2-res0-not-res1", 2, 4, 8, 0, 8, 8, 32, (2, 1, 1, 1), res=(8, 8), bmod=(0, 0, 2, 0)),
    Case("bmod-rp7-B8m2", 7, 8, 8, 0, 8, 8, 32, (3, 1, 2, 1), res="id", bmod=(2, 0, 2, 0)),          # b >= 2 bmod: mi_row_of's b % bmod branch
    Case("bmod-stripe-8+8-fallback", 12, 4, 8, 8, 8, 16, 64, (130, 3, 1, 1), bmod=(2, 0, 0, 0)),     # the row of mi_gn_channel_totals (stripe fallback)
    Case("bmod-wide7-res-conv", 7, 4, 32, 32, 32, 8, 32, (3, 2, 2, 3), res=(32, 32), bmod=(2, 0, 2, 0), wide=True),      # conv_wide.hip:68 is the GEMM's; this is gn_coef's residual side
    Case("bmod-gemm11-res-conv", 11, 4, 32, 32, 64, 8, 16, (3, 2, 2, 3), res=(32, 32), bmod=(2, 0, 2, 0)),              # mi_conv_prep_fwd's rows of both operands
]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", BMOD_CASES, ids=str)
def test_shared_batch_rows(backend, case):
    """B: mi_act.bmod on in0 and res0 together and separately (and on one half of a concat only), with multi-tile statistics: the tensor holds
    bmod rows, what follows them in the allocation is 1e30, the reference expands the rows.  Output rows b and b + bmod must differ."""
    run_case(backend, case)


# ---------------------------------------------------------------------------------------------------------------------------------
# C. the engine's flag words on the direct family at the sizes of the 20 x 20 plan.  mi_conv_fwd's direct dispatch by (form, cout tile, flags):
#    k3:   <4,3,1,false> for Cout <= 4 and for Cout 8 with SPLIT8; <8,3,1,false> for a cout tile of 8 and for 16 with SPLIT16; <16,3,1,false>
#    up2:  <16,3,1,true>; <8,3,1,true> without SPLIT8; <4,3,1,true> for Cout <= 4 and Cout 8 with SPLIT8
#    k4s2: <8,4,2,false> for cout tiles 16 and 8 without SPLIT8; <4,4,2,false> for Cout <= 4 and Cout 8 with SPLIT8

DIRECT_CASES = [
    Case("direct-k3-8-20x20", 2, 2, 8, 0, 8, 20, 20, (3, 1, 1, 1), res="id"),
    Case("direct-k3-8-6x10-res-conv", 2, 2, 8, 8, 8, 6, 10, (2, 3, 1, 1), res=(8, 8)),
    Case("direct-up2-8-10x10", 2, 2, 16, 0, 8, 10, 10, (2, 1, 1, 1), mode="up2", gn=False),
    Case("direct-k4s2-8-5x5", 2, 2, 8, 0, 8, 5, 5, (3, 1, 1, 1), mode="k4s2", gn=False),
    Case("direct-k4s2-8-10x10", 2, 2, 8, 0, 8, 10, 10, (3, 1, 1, 1), mode="k4s2", gn=False),          # the recorded 0x902 launch: 10 x 10 from 20 x 20
    Case("direct-k3-16-10x10", 2, 2, 16, 0, 16, 10, 10, (2, 1, 1, 1), res="id"),
    Case("direct-k3-16-20x20-res-conv", 2, 2, 16, 8, 16, 20, 20, (3, 2, 1, 1), res=(16, 8)),
    Case("direct-up2-16-10x10", 2, 2, 16, 0, 16, 10, 10, (2, 1, 1, 1), mode="up2", gn=False),
    Case("direct-k4s2-16-5x5", 2, 2, 8, 0, 16, 5, 5, (3, 1, 1, 1), mode="k4s2", gn=False),
    Case("direct-k3-3-20x20", 2, 2, 8, 0, 3, 20, 20, (3, 1, 1, 1)),
    Case("direct-up2-3-10x10", 2, 2, 8, 0, 3, 10, 10, (2, 1, 1, 1), mode="up2", gn=False),
    Case("direct-k4s2-3-5x5", 2, 2, 8, 0, 3, 5, 5, (3, 1, 1, 1), mode="k4s2", gn=False),
    Case("direct-k3-24-6x10", 2, 2, 16, 0, 24, 6, 10, (2, 1, 1, 1), res=(8, 0)),           # three 8-channel tiles
    Case("direct0-k3-8-20x20", 0, 2, 8, 0, 8, 20, 20, (3, 1, 1, 1), res="id"),
    Case("direct0-k3-16-6x10", 0, 2, 16, 0, 16, 6, 10, (2, 1, 1, 1), res="id"),
    Case("direct-k3-8-12x20-vec", 2, 2, 8, 0, 8, 12, 20, (3, 1, 1, 1), res="id"),          # W % 4 == 0: the vector staging under the same flags
]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", DIRECT_CASES, ids=str)
def test_direct_family_engine_words(backend, case):
    """C: every direct-conv instantiation the engine's word selects, at 20 x 20 / 10 x 10 / 5 x 5 / 6 x 10, against fp64 with the bare tile
    code, and bit for bit the same with | MI_CONV_SPLIT16 | MI_CONV_SPLIT8 (0x902 / 0x900 as conv_route.tile_word builds it) and with each flag
    alone: the flags only choose how many output channels a workgroup takes; every output channel is one accumulator that walks the input
    channels and taps in the same order, and its statistics are reduced over the same work-items, whatever the channel tile."""
    run_case(backend, case, words=(case.code | ENGINE, case.code | SPLIT16, case.code | SPLIT8))


# ---------------------------------------------------------------------------------------------------------------------------------
# D. placement-only flags

@functools.lru_cache(maxsize=None)
def recorded_words():
    """the distinct tile_cfg words of the MiConvParams lines of the recorded plans"""
    words = set()
    with gzip.open(PLANS, "rt") as f:
        for line in f:
            if "MiConvParams" in line:
                words.update(int(m) for m in re.findall(r"\btile_cfg=(\d+)", line))
    assert words, "no conv launch in the recorded plans"
    return frozenset(words)


PLACEMENT_CASES = [
    # B = 8: the XCD-aware workgroup -> image map, which MI_CONV_REVERSE walks backwards
    Case("place-rp6", 6, 8, 8, 0, 8, 24, 128, (3, 1, 2, 1), res="id"),                     # 6 tiles: strips of 1, 2, 3, 6 divide; 4, 5 do not; 7 .. 15 > tiles
    Case("place-rp6-16", 6, 8, 16, 0, 16, 16, 64, (3, 1, 2, 1), res="id"),                 # 16 output channels: two N tiles under SPLIT16
    Case("place-rp7", 7, 8, 8, 0, 8, 24, 64, (3, 1, 2, 1), res="id"),
    Case("place-rp7-k4s2", 7, 8, 8, 0, 16, 8, 64, (3, 1, 1, 1), mode="k4s2", gn=False),
    Case("place-half6", 6, 8, 8, 0, 8, 16, 128, (3, 1, 2, 1), res="id", half=True),
    Case("place-half7", 7, 8, 8, 0, 8, 16, 64, (3, 1, 2, 1), res="id", half=True),
    Case("place-wide6", 6, 8, 32, 0, 32, 8, 64, (3, 1, 2, 1), res="id", wide=True),
    Case("place-wide7", 7, 8, 32, 0, 32, 8, 32, (3, 1, 2, 1), res="id", wide=True),
    Case("place-wide10", 10, 8, 32, 0, 32, 16, 16, (3, 1, 2, 1), res="id", wide=True),
    Case("place-gemm11", 11, 8, 32, 0, 64, 16, 16, (3, 1, 2, 1), res="id"),
    Case("place-stripe", 12, 8, 8, 0, 8, 32, 64, (3, 1, 2, 1), res="id"),                  # 4 statistics blocks: 1, 2, 4 divide
    Case("place-stripe-16", 12, 8, 16, 0, 16, 16, 64, (3, 1, 2, 1), res="id"),
    Case("place-stripe-k4s2", 12, 8, 8, 0, 16, 16, 64, (3, 1, 1, 1), mode="k4s2", gn=False),
]


def placement_words(c: Case):
    """every word that must give the bits of the bare code (with | 0x400 where the case is a single-term one): REVERSE, every strip count,
    the engine's split flags, their combinations -- and every recorded word of the case's code and precision"""
    base = c.word
    words = {base | REVERSE, base | ENGINE, base | SPLIT16, base | ENGINE | REVERSE}
    words |= {base | (n << 12) for n in range(1, 16)}
    words |= {base | REVERSE | (n << 12) for n in (2, 3)}
    words |= {w for w in recorded_words() if (w & 0xff) == c.code and bool(w & HALF) == c.half}
    return sorted(words - {base})


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", PLACEMENT_CASES, ids=str)
def test_placement_flags_leave_the_bits_alone(backend, case):
    """D: tile codes 6, 7, 10, 11 (and 12, as test_conv_stripe.py has it for two words) at B = 8: MI_CONV_REVERSE, every strip count n << 12
    whether it divides the tile count or not, MI_CONV_SPLIT16 | MI_CONV_SPLIT8 and the exact words of the recorded plans all give torch.equal
    outputs and statistics to the bare code."""
    run_case(backend, case, words=placement_words(case))


ALL_CASES = MULTI_TILE_CASES + BMOD_CASES + DIRECT_CASES + PLACEMENT_CASES          # (part E's launches are listed below and added there)


def launched_words():
    """tile_cfg word -> the cases of this file that launch it"""
    table = {}
    for c in ALL_CASES:
        ws = {c.word}
        if c in DIRECT_CASES:
            ws |= {c.code | ENGINE, c.code | SPLIT16, c.code | SPLIT8}
        if c in PLACEMENT_CASES:
            ws |= set(placement_words(c))
        for w in ws:
            table.setdefault(w, []).append(c)
    return table


def test_every_recorded_word_has_an_op_level_case():
    """every distinct tile_cfg word of tests/golden/conv_plans.txt.gz is launched by a case of this file (on a shape its family admits: the
    case's own test launches it through L.check), and every tile code of the snapshot has a case with nt > 1 and one with bmod > 0.  A new word
    in the snapshot fails here until it has an op-level case."""
    table = launched_words()
    missing = sorted(w for w in recorded_words() if w not in table)
    assert not missing, f"recorded tile_cfg words without an op-level case: {[hex(w) for w in missing]}"
    for code in sorted({w & 0xff for w in recorded_words()}):
        mine = [c for c in ALL_CASES if c.code == code]
        assert any(max(c.nt) > 1 and c.nt[0] > 1 for c in mine), f"tile code {code}: no case with multi-tile statistics"
        assert any(max(c.bmod) > 0 for c in mine), f"tile code {code}: no case with bmod"
    print(f"{len(recorded_words())} recorded words, {len(table)} launched: {[hex(w) for w in sorted(recorded_words())]}")


# ---------------------------------------------------------------------------------------------------------------------------------
# E. statistics hand-offs between families: conv 1 writes y1 and out_stats [B][C][out_nt][2]; conv 2 (GroupNorm + scale / shift + SiLU + conv)
#    consumes y1 with stats = conv 1's out_stats, nt = conv 1's out_nt.

HANDOFF_PAIRS = [
    # (producer, consumer): the consumer's C0 / input size are the producer's Cout / output size; its nt[0] is replaced by the producer's out_nt
    (Case("E-direct2", 2, 2, 8, 0, 8, 16, 32, (3, 1, 1, 1)), Case("E-direct2->rp7", 7, 2, 8, 0, 8, 16, 32)),
    (Case("E-rp6", 6, 2, 8, 0, 8, 16, 64, (3, 1, 1, 1)), Case("E-rp6->stripe", 12, 2, 8, 0, 8, 16, 64)),
    (Case("E-stripe", 12, 2, 8, 0, 8, 16, 32, (3, 1, 1, 1)), Case("E-stripe->rp7", 7, 2, 8, 0, 8, 16, 32)),
    (Case("E-stripe-k4s2", 12, 2, 8, 0, 16, 16, 64, (3, 1, 1, 1), mode="k4s2", gn=False), Case("E-stripe-k4s2->rp7", 7, 2, 16, 0, 16, 16, 64)),
    (Case("E-rp7", 7, 2, 8, 0, 8, 16, 32, (3, 1, 1, 1)), Case("E-rp7->direct2", 2, 2, 8, 0, 8, 16, 32)),
    (Case("E-gemm11", 11, 2, 32, 0, 64, 8, 32, (3, 1, 1, 1)), Case("E-gemm11->wide7", 7, 2, 64, 0, 32, 8, 32, wide=True)),
    (Case("E-stripe-strips2", 12, 8, 8, 0, 8, 16, 64, (3, 1, 1, 1), flags=2 << 12), Case("E-stripe-strips2->stripe-rev", 12, 8, 8, 0, 8, 16, 64, flags=REVERSE)),
]
ALL_CASES += [c for pair in HANDOFF_PAIRS for c in pair]


def per_tile_sums(y, tile):
    """fp64 (sum, sum of squares) of y [B][C][H][W] over th x tw tiles in row-major tile order -> [B][C][nt][2] and the pixels of each tile"""
    th, tw = tile
    B, Cc, H, W = y.shape
    y = y.double()
    recs, counts = [], []
    for y0 in range(0, H, th):
        for x0 in range(0, W, tw):
            blk = y[:, :, y0:y0 + th, x0:x0 + tw]
            recs.append(torch.stack((blk.sum((2, 3)), (blk ** 2).sum((2, 3))), -1))
            counts.append(blk.shape[2] * blk.shape[3])
    return torch.stack(recs, 2), torch.tensor(counts, dtype=torch.float64)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("pair", HANDOFF_PAIRS, ids=lambda pr: pr[1].name)
def test_statistics_hand_off(backend, pair):
    """E: two launches through the C ABI.  Conv 1 against its own fp64 reference; its out_stats PER TILE against fp64 sums over that tile's
    pixels of the y1 it wrote (check_stats only sees the totals, which do not notice a record in the wrong slot); conv 2 against fp64 of the
    Block applied to the kernel's ACTUAL y1 -- exact in fp64, so only the statistics' accuracy and layout are under test and the family's gate
    applies unchanged.
    The per-tile bound: test_block_bwd_ops' bound for its chunk records (n 2^-52 sum |x|) belongs to a kernel that adds in fp64 throughout; the
    convs' epilogues add a work-item's few values in fp32 about a local shift and go to fp64 from there (common.hip.h, mi_stat_acc), so the bound
    here is relative 1e-6 of the tile's sum of squares for Q and, for S, 1e-6 sqrt(n Q) >= 1e-6 sum |x| (Cauchy-Schwarz): a few fp32 roundings
    (2^-24 = 6e-8 each) of partial sums that never exceed sum |x| resp. Q."""
    c1, c2 = pair
    dev = setup(backend)
    t1 = host_case(c1)
    p1 = Prepared(dev, c1, t1)
    y1, st1 = p1.run(c1.word)
    y1b, st1b = p1.run(c1.word)
    what = f"{c2} [{backend}]"
    assert torch.equal(bits(y1), bits(y1b)) and torch.equal(bits(st1), bits(st1b)), f"{what}: two runs of conv 1 differ"
    gate(f"{what} conv 1", c1, y1, st1, t1["ref"], t1["yard"])
    assert p1.out_nt > 1, f"{what}: the producer leaves one tile, the pair exercises no multi-tile read"
    y1h, st1h = y1.cpu(), st1.cpu()
    want, n = per_tile_sums(y1h, p1.tile)
    assert want.shape == st1h.shape
    eS = ((st1h[..., 0] - want[..., 0]).abs() / (1e-6 * (n * want[..., 1]).sqrt())).max().item()
    eQ = ((st1h[..., 1] - want[..., 1]).abs() / (1e-6 * want[..., 1])).max().item()
    print(f"{what} conv 1 out_stats per tile ({p1.out_nt} tiles of {p1.tile[0]} x {p1.tile[1]}): |dS| / bound {eS:.3f}, |dQ| / bound {eQ:.3f}")
    assert eS <= 1.0 and eQ <= 1.0, (what, eS, eQ)
    # conv 2 on the kernel's y1 and ITS statistics buffer (the device tensors of launch 1 stay alive in p1.last)
    c2 = c2._replace(nt=(p1.out_nt, 1, 1, 1))
    t2 = tensors_of(c2)
    assert t2["x0"].shape == (c2.B, c2.C0, c2.H * c2.W) and y1h.shape == (c2.B, c2.C0, c2.H, c2.W)
    t2["x0"] = y1h.reshape(t2["x0"].shape)
    t2["ref"], t2["yard"] = reference(c2, t2, torch.float64), reference(c2, t2, torch.float32)
    p2 = Prepared(dev, c2, t2)
    p2.p.in0 = L.MiAct(y1.data_ptr(), c2.C0, st1.data_ptr(), p1.out_nt, 1.0, 0, 0)
    y2, st2 = p2.run(c2.word)
    y2b, st2b = p2.run(c2.word)
    assert torch.equal(bits(y2), bits(y2b)) and torch.equal(bits(st2), bits(st2b)), f"{what}: two runs of conv 2 differ"
    gate(f"{what} conv 2", c2, y2, st2, t2["ref"], t2["yard"])
