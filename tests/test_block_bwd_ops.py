"""Op-level fp64 parity of the training backward of ``Block`` (GroupNorm -> [scale / shift] -> SiLU -> Conv3x3, layers.py:107-145), which is
otherwise reached only through test_block_function_gradients and the whole-U-Net step tests:

A  mi_chan_stats_fwd (train_bwd.hip): the fp64 channel statistics, vector and scalar path;
B  mi_block_bwd (train_bwd.hip), called directly: batch walks past one wave, chunked rows, multi-tile statistics, ss_off / ss_stride;
C  mi_conv_wgrad (conv_wgrad.hip) with the activation fused into its operand staging (a_stats != NULL);
D  the data-gradient conv -- mi_conv_fwd on the adjoint pack through train_ops._conv3x3 -- over per-image gradient magnitudes that differ by
   orders of magnitude inside one launch, and at both ends of its documented domain;
E  the hand-offs between two stacked Blocks: out_stats forward, dx_stats backward, and the version guards on both.

Every reference is fp64 torch autograd on the CPU.  The exact-fp32-product kernels (B, C, and the parameter gradients of E) are held to
test_attn_ops' yardstick: 4 x the error of the same formula in fp32 torch ops on the CPU + 4 fp32 ulps of max |ref|.  The fp16 hi|lo
convolutions (D, and y / dx of E) are held to the conv family's own gate of test_kernels, err < 2e-5 * scale, PER IMAGE with
scale = max |ref[b]|; their yardstick ratio is printed only.  Outputs and workspaces are pre-filled with NaN and followed by a canary, every
launch runs twice and must repeat its bits."""
import copy
import ctypes as C
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from minimagen_amd import _lib as L, train_ops
from minimagen_amd.layers import Block
from tests._backend import BACKENDS, setup

MI_ERR_INVALID = -1
EPS = 1e-5
CANARY, SENTINEL = 16, 12345


def f32_ulp(v: float) -> float:
    """spacing of fp32 at magnitude v"""
    return 2.0 ** (math.floor(math.log2(max(v, 2.0 ** -126))) - 23)


def within_yardstick(what, out, ref, yard_out):
    """max |kernel - fp64| <= 4 x max |fp32 torch - fp64| + 4 fp32 ulps of max |fp64|; prints kernel error / yardstick (test_attn_ops)"""
    assert torch.isfinite(out).all(), f"{what}: output not finite / not fully written"
    err = (out.double() - ref).abs().max().item()
    yard = (yard_out.double() - ref).abs().max().item()
    refmax = ref.abs().max().item()
    tol = 4.0 * yard + 4.0 * f32_ulp(refmax)
    print(f"{what}: max|d| {err:.2e}, yardstick {yard:.2e}, |ref|max {refmax:.3g}, kernel error / yardstick {err / max(yard, 1e-30):.2f}, error / tolerance {err / tol:.2f}")
    assert err <= tol, (what, err, yard, tol)


def conv_gate_per_image(what, out, ref, yard_out):
    """the conv family's gate (test_kernels: err < 2e-5 * scale) per image with scale = max |ref[b]|: an image whose gradient is orders of
    magnitude below its neighbours' is held to its OWN magnitude.  An all-zero reference image must come back as exact zeros.  Prints the
    error relative to the image's maximum and against the fp32 yardstick (not gated).  Returns the relative errors."""
    assert torch.isfinite(out).all(), f"{what}: output not finite / not fully written"
    rels = []
    for b in range(ref.shape[0]):
        scale = ref[b].abs().max().item()
        err = (out[b].double() - ref[b]).abs().max().item()
        if scale == 0.0:
            assert err == 0.0 and not out[b].any(), f"{what}: image {b} has a zero reference, the kernel wrote non-zeros"
            print(f"{what} image {b}: all zeros")
            rels.append(0.0)
            continue
        yard = (yard_out[b].double() - ref[b]).abs().max().item()
        print(f"{what} image {b}: |ref|max {scale:.3g}, error / |ref|max {err / scale:.2e} (gate 2e-5), fp32 torch {yard / scale:.2e}, kernel error / yardstick {err / max(yard, 1e-300):.2f}")
        assert err < 2e-5 * scale, (what, b, err, scale)
        rels.append(err / scale)
    return rels


def guarded(shape, dtype, dev):
    """a buffer of prod(shape) elements pre-filled with NaN (integers: the type's minimum), followed by CANARY sentinel elements"""
    n = math.prod(shape)
    flat = torch.empty(n + CANARY, dtype=dtype, device=dev)
    flat[:n] = float('nan') if dtype.is_floating_point else torch.iinfo(dtype).min
    flat[n:] = SENTINEL
    # (not flat[:n].view(shape): to autograd the buffers train_ops allocates are tensors of their own, not views of another one)
    return flat, torch.empty(0, dtype=dtype, device=dev).set_(flat.untyped_storage(), 0, tuple(shape))


def canary_intact(flat):
    return bool((flat[-CANARY:] == SENTINEL).all())


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def group_act(x, gamma, beta, scale, shift, groups):
    """SiLU(GroupNorm(x) * (scale + 1) + shift) in the dtype of its arguments (layers.py:131-145 without the conv): x [B][C][...],
    gamma / beta [C], scale / shift [B][C] or None; biased variance, eps inside the root"""
    B, Cc = x.shape[:2]
    xg = x.reshape(B, groups, -1)
    mu = xg.mean(-1, keepdim=True)
    var = ((xg - mu) ** 2).mean(-1, keepdim=True)
    xh = ((xg - mu) / torch.sqrt(var + EPS)).reshape(x.shape)
    pc, pb = (1, Cc) + (1,) * (x.dim() - 2), (B, Cc) + (1,) * (x.dim() - 2)
    y = xh * gamma.reshape(pc) + beta.reshape(pc)
    if scale is not None:
        y = y * (scale.reshape(pb) + 1) + shift.reshape(pb)
    return F.silu(y)


def unequal_cuts(n, pieces, g):
    """0 = c_0 < c_1 < ... < c_pieces = n at random places: statistics tiles of different sizes"""
    inner = sorted((torch.randperm(n - 1, generator=g)[:pieces - 1] + 1).tolist()) if pieces > 1 else []
    return [0] + inner + [n]


def piece_stats(x, cuts):
    """fp64 (sum, sum of squares) of x [B][C][n] over the pieces cuts[t] .. cuts[t + 1] -> [B][C][nt][2]: what a producing conv's epilogue leaves"""
    x64 = x.double()
    return torch.stack([torch.stack((x64[..., a:b].sum(-1), (x64[..., a:b] ** 2).sum(-1)), -1) for a, b in zip(cuts[:-1], cuts[1:])], 2).contiguous()


def chunk_stats(x, nchunk):
    """the records mi_block_bwd leaves for its dx: per = ceil(n / nchunk) elements per chunk, the last ragged or empty"""
    n = x.shape[-1]
    per = -(-n // nchunk)
    return piece_stats(x, [min(j * per, n) for j in range(nchunk + 1)])


def offset_input(rn, g, B, Cc, n, off):
    """1.5 sigma noise around per-channel offsets of 0.5 .. 1 x `off` sigma of either sign"""
    u = (0.5 + 0.5 * torch.rand(Cc, generator=g)) * (2.0 * torch.randint(0, 2, (Cc,), generator=g) - 1.0)
    return 1.5 * (rn(B, Cc, n) + off * u[None, :, None])


def ss_table(B, Cc, scale, shift, stride, off):
    """[B][stride] with the scale at off + c and the shift at off + C + c; every other entry is 1e3, so that a misplaced read is far off"""
    tab = torch.full((B, stride), 1e3)
    tab[:, off:off + Cc], tab[:, off + Cc:off + 2 * Cc] = scale, shift
    return tab


# ---------------------------------------------------------------------------------------------------------------------------------
# A. mi_chan_stats_fwd

# (rows, HW, added mean, element offset of the pointer into a 16-byte-aligned buffer)
CHAN_STATS_CASES = [(5, 4096, 0, 0),          # vector path
                    (5, 4099, 1000, 0),       # scalar path by HW
                    (3, 4096, 1000, 1),       # scalar path by alignment
                    (7, 3, 5, 0),             # fewer elements than work-items
                    (2, 4100, 100, 0),        # vector path, last stride partial (1025 float4)
                    (1, 1, 2, 0)]
# Depth of the kernel's summation: every work-item adds at most ceil(HW / 1024) <= 5 elements in sequence (vector path: <= 2 steps of a
# three-level sum), then 6 shuffle levels, then 16 wave sums in sequence: no element passes through more than D = 32 fp64 additions, each
# rounding by at most u = 2^-53 of the running sum: |dS| <= D u sum |x|, |dQ| <= D u Q (the fma adds one rounding per step, counted in D).
# var = Q / n - (S / n)^2 then moves by |dQ| / n + 2 |m| |dS| / n <= 3 D u Q / n (|m| sum |x| <= Q by Cauchy-Schwarz), and evaluating the
# expression itself in fp64 rounds by <= 3 u Q / n:  |d var| <= (3 D + 3) u Q / n = 49.5 * 2^-52 Q / n.  VAR_CONST is the next power of two.
VAR_CONST = 64.0


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", CHAN_STATS_CASES, ids=lambda c: "x".join(map(str, c)))
def test_chan_stats(backend, case):
    """mi_chan_stats_fwd against fp64 sums: |S - S64| <= HW 2^-52 sum |x| and |Q - Q64| <= HW 2^-52 sum x^2 (the bound of fp64 summation in any
    order), and the variance derived from the record against the two-pass fp64 variance within VAR_CONST 2^-52 Q / (HW var) relative -- with a
    mean of 1000 sigma that is 1e-8 of the variance, where an fp32 sum of squares keeps no digit of it (the kernel's "large mean" comment).
    The vector path (HW % 4 == 0 and a 16-byte-aligned pointer) and the scalar path by either condition; bad arguments are refused."""
    rows, HW, mean, off = case
    dev = setup(backend)
    lib = L.lib()
    g = torch.Generator().manual_seed(rows * 10007 + HW)
    x = torch.randn(rows, HW, generator=g) + float(mean)
    base = torch.zeros(rows * HW + 4, device=dev)
    assert base.data_ptr() % 16 == 0
    xd = base[off:off + rows * HW]
    xd.copy_(x.reshape(-1))
    x64 = x.double()
    S64, Q64, A64 = x64.sum(-1), (x64 ** 2).sum(-1), x64.abs().sum(-1)
    var64 = ((x64 - x64.mean(-1, keepdim=True)) ** 2).mean(-1)
    runs = []
    for _ in range(2):
        flat, st = guarded((rows, 2), torch.float64, dev)
        L.check(lib.mi_chan_stats_fwd(xd.data_ptr(), st.data_ptr(), rows, HW, L.current_stream()), "mi_chan_stats_fwd")
        flat = flat.cpu()
        assert canary_intact(flat), "the elements after stats were overwritten"
        runs.append(flat[:rows * 2].view(rows, 2))
    st = runs[0]
    assert torch.isfinite(st).all() and torch.equal(bits(runs[0]), bits(runs[1]))
    eS = ((st[:, 0] - S64).abs() / (HW * 2.0 ** -52 * A64)).max().item()
    eQ = ((st[:, 1] - Q64).abs() / (HW * 2.0 ** -52 * Q64)).max().item()
    var = st[:, 1] / HW - (st[:, 0] / HW) ** 2
    bound = VAR_CONST * 2.0 ** -52 * Q64 / HW
    eV = ((var - var64).abs() / bound).max().item()
    print(f"chan-stats {backend} {case}: |dS| / bound {eS:.2e}, |dQ| / bound {eQ:.2e}, |d var| / bound {eV:.2e}; "
          f"bound / var {(bound / var64.clamp_min(1e-300)).max().item():.1e}")
    assert eS <= 1.0 and eQ <= 1.0 and eV <= 1.0, (case, eS, eQ, eV)
    flat, st = guarded((rows, 2), torch.float64, dev)
    for args in ((0, st.data_ptr(), rows, HW), (xd.data_ptr(), 0, rows, HW), (xd.data_ptr(), st.data_ptr(), 0, HW), (xd.data_ptr(), st.data_ptr(), rows, 0),
                 (xd.data_ptr(), st.data_ptr(), -1, HW), (xd.data_ptr(), st.data_ptr(), rows, -4)):
        assert lib.mi_chan_stats_fwd(*args, L.current_stream()) == MI_ERR_INVALID
    assert torch.isnan(flat[:rows * 2]).all() and canary_intact(flat.cpu()), "a refused call wrote"


# ---------------------------------------------------------------------------------------------------------------------------------
# B. mi_block_bwd

# (B, C, HW, groups, nchunk, nt, scale/shift, channel offsets in sigma, (ss_stride - 2C, ss_off))
BLOCK_BWD_CASES = [
    (2, 8, 64, 8, 1, 1, True, 0, (0, 0)),
    (3, 24, 1000, 3, 3, 1, True, 0, (0, 0)),          # per = 334: the last chunk holds 332
    (3, 24, 1000, 3, 3, 5, True, 30, (0, 0)),         # 5 statistics tiles of unequal size per channel
    (2, 12, 1027, 4, 4, 3, False, 30, (0, 0)),        # per = 257: one element past the 256 work-items; last chunk 256
    (70, 8, 50, 2, 1, 1, True, 1, (0, 0)),            # the parameter kernel's lanes take a second image (b = lane + 64)
    (2, 16, 2050, 1, 2, 1, True, 300, (0, 0)),        # one group over all channels, offsets of 300 sigma
    (1, 4, 5, 4, 3, 1, True, 0, (0, 0)),              # per = 2: chunks of 2, 2, 1 elements
    (1, 4, 5, 4, 4, 1, True, 0, (0, 0)),              # per = 2: the fourth chunk is empty and must record (0, 0)
    (2, 130, 40, 2, 1, 2, True, 3, (0, 0)),           # cpg * nt = 130 > 64 statistics records per group (group moments walk twice)
    (2, 32, 300, 1, 3, 1, True, 3, (0, 0)),           # cpg * nchunk = 96 > 64 row sums per group (the apply kernel's group means walk twice)
    (3, 24, 1000, 3, 3, 1, True, 0, (7, 3)),          # ss_stride = 2C + 7, ss_off = 3
]


@functools.lru_cache(maxsize=None)
def block_bwd_case(B, Cc, HW, groups, nt, with_ss, off):
    """inputs, statistics tiles, the fp64 gradients and the fp32 yardstick of one case (shared by both backends and the ss layouts)"""
    g = torch.Generator().manual_seed(B * 1000003 + Cc * 1009 + HW + nt)
    rn = lambda *s: torch.randn(*s, generator=g)
    x = offset_input(rn, g, B, Cc, HW, off)
    da = rn(B, Cc, HW)
    gamma, beta = 1 + 0.3 * rn(Cc), 0.2 * rn(Cc)
    scale, shift = (0.3 * rn(B, Cc), 0.3 * rn(B, Cc)) if with_ss else (None, None)
    out = dict(x=x, da=da, gamma=gamma, beta=beta, scale=scale, shift=shift, stats=piece_stats(x, unequal_cuts(HW, nt, g)))
    for key, dt in (("ref", torch.float64), ("yard", torch.float32)):
        leaves = [t.to(dt).clone().requires_grad_() for t in (x, gamma, beta) + ((scale, shift) if with_ss else ())]
        a = group_act(leaves[0], leaves[1], leaves[2], *(leaves[3:] if with_ss else (None, None)), groups)
        gr = torch.autograd.grad((a * da.to(dt)).sum(), leaves)
        out[key] = dict(dx=gr[0], dgamma=gr[1], dbeta=gr[2], dss=torch.cat(gr[3:], 1) if with_ss else None)
    return out


def run_block_bwd(dev, case, B, Cc, HW, groups, nchunk, nt, ss_pad, ss_off, want_stats):
    """one mi_block_bwd call through L.MiBlockBwdParams on guarded buffers -> the outputs on the host"""
    keep = {k: case[k].to(dev).contiguous() for k in ("x", "da", "gamma", "beta", "stats")}
    with_ss = case["scale"] is not None
    bufs = dict(uv=guarded((B, Cc, nchunk, 2), torch.float32, dev), dx=guarded((B, Cc, HW), torch.float32, dev),
                dgamma=guarded((Cc,), torch.float32, dev), dbeta=guarded((Cc,), torch.float32, dev))
    if with_ss:
        bufs["dss"] = guarded((B, 2 * Cc), torch.float32, dev)
        keep["ss"] = ss_table(B, Cc, case["scale"], case["shift"], 2 * Cc + ss_pad, ss_off).to(dev)
    if want_stats:
        bufs["dx_stats"] = guarded((B, Cc, nchunk, 2), torch.float64, dev)
    p = L.MiBlockBwdParams()
    p.B, p.C, p.HW, p.groups, p.nt, p.nchunk, p.eps = B, Cc, HW, groups, nt, nchunk, EPS
    p.x, p.da, p.x_stats, p.gamma, p.beta = [keep[k].data_ptr() for k in ("x", "da", "stats", "gamma", "beta")]
    if with_ss:
        p.ss, p.ss_stride, p.ss_off = keep["ss"].data_ptr(), 2 * Cc + ss_pad, ss_off
    for k, (_, view) in bufs.items():
        setattr(p, k, view.data_ptr())
    L.check(L.lib().mi_block_bwd(C.byref(p), L.current_stream()), "mi_block_bwd")
    out = {}
    for k, (flat, view) in bufs.items():
        flat = flat.cpu()
        assert canary_intact(flat), f"the elements after {k} were overwritten"
        out[k] = flat[:view.numel()].view(view.shape)
    return out


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", BLOCK_BWD_CASES, ids=lambda c: "x".join(map(str, c[:6])) + ("-ss" if c[6] else "") + f"-off{c[7]}" + ("-sslayout" if c[8] != (0, 0) else ""))
def test_block_bwd_kernel(backend, case):
    """mi_block_bwd against fp64 autograd of SiLU(GroupNorm(x) (scale + 1) + shift): dx, dgamma, dbeta and d(scale | shift) within the fp32
    yardstick; dx_stats[b][c][j] against fp64 sums over chunk j (per = ceil(HW / nchunk)) of the kernel's OWN dx within the fp64 summation bound
    n 2^-52 sum |dx| -- compared per chunk, since a total would not notice a record in the wrong slot; the same call with dx_stats = NULL
    writes the same bits.  x_stats arrive as nt tiles of unequal size, built in fp64 on the host."""
    B, Cc, HW, groups, nchunk, nt, with_ss, off, (ss_pad, ss_off) = case
    dev = setup(backend)
    what = f"block-bwd {backend} B{B} C{Cc} HW{HW} g{groups} nchunk{nchunk} nt{nt} off{off}" + (f" ss+{ss_pad}@{ss_off}" if with_ss else "")
    ref = block_bwd_case(B, Cc, HW, groups, nt, with_ss, off)
    runs = [run_block_bwd(dev, ref, B, Cc, HW, groups, nchunk, nt, ss_pad, ss_off, True) for _ in range(2)]
    runs.append(run_block_bwd(dev, ref, B, Cc, HW, groups, nchunk, nt, ss_pad, ss_off, False))
    names = ["dx", "dgamma", "dbeta"] + (["dss"] if with_ss else [])
    for k in names + ["uv", "dx_stats"]:
        assert torch.equal(bits(runs[0][k]), bits(runs[1][k])), f"{what}: {k} differs between two runs"
    for k in names:
        assert torch.equal(bits(runs[0][k]), bits(runs[2][k])), f"{what}: {k} differs without dx_stats"
        within_yardstick(f"{what} {k}", runs[0][k], ref["ref"][k], ref["yard"][k])
    assert torch.isfinite(runs[0]["uv"]).all(), f"{what}: a row-sum record was not written"
    dxs, dx64 = runs[0]["dx_stats"], runs[0]["dx"].double()
    assert torch.isfinite(dxs).all(), f"{what}: a dx_stats record was not written"
    per = -(-HW // nchunk)
    worst = 0.0
    for j in range(nchunk):
        sl = dx64[:, :, j * per:(j + 1) * per]
        n = sl.shape[-1]
        if n == 0:
            assert not dxs[:, :, j].any(), f"{what}: the empty chunk {j} does not record (0, 0)"
            continue
        eS = (dxs[:, :, j, 0] - sl.sum(-1)).abs() / (n * 2.0 ** -52 * sl.abs().sum(-1)).clamp_min(1e-300)
        eQ = (dxs[:, :, j, 1] - (sl ** 2).sum(-1)).abs() / (n * 2.0 ** -52 * (sl ** 2).sum(-1)).clamp_min(1e-300)
        worst = max(worst, eS.max().item(), eQ.max().item())
    print(f"{what}: dx_stats per chunk, worst deviation / fp64 summation bound {worst:.2e}; chunks of {per}, the last of {HW - (nchunk - 1) * per}")
    assert worst <= 1.0, (what, worst)


@pytest.mark.parametrize("backend", BACKENDS)
def test_block_bwd_rejections(backend):
    """argument checks of mi_block_bwd: refused before any device work, nothing written"""
    dev = setup(backend)
    lib = L.lib()
    B, Cc, HW = 2, 8, 16
    flat, buf = guarded((5, B * Cc * HW), torch.float32, dev)
    fill = torch.zeros(B * Cc * HW, dtype=torch.float64, device=dev)

    def params(**kw):
        p = L.MiBlockBwdParams()
        p.B, p.C, p.HW, p.groups, p.nt, p.nchunk, p.eps = B, Cc, HW, 4, 1, 1, EPS
        p.x = p.da = p.gamma = p.beta = p.ss = p.x_stats = fill.data_ptr()
        p.ss_stride = 2 * Cc
        p.uv, p.dx, p.dgamma, p.dbeta, p.dss = [buf[i].data_ptr() for i in range(5)]
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    for bad in (dict(groups=3), dict(groups=0), dict(nchunk=0), dict(nchunk=65536), dict(nt=0), dict(dss=None), dict(B=0), dict(HW=0), dict(x_stats=None),
                dict(uv=None), dict(dx=None), dict(dgamma=None), dict(dbeta=None)):
        assert lib.mi_block_bwd(C.byref(params(**bad)), L.current_stream()) == MI_ERR_INVALID, bad
    assert lib.mi_block_bwd(None, L.current_stream()) == MI_ERR_INVALID
    assert torch.isnan(buf).all() and canary_intact(flat.cpu())
    L.check(lib.mi_block_bwd(C.byref(params(ss=None, dss=None)), L.current_stream()), "mi_block_bwd without scale / shift and without dss")


# ---------------------------------------------------------------------------------------------------------------------------------
# C. mi_conv_wgrad with the activation fused into the staging of its A operand

# (B, Cin, Cout, H, W, groups, nwg, a_nt, scale/shift, channel offsets in sigma, (ss_stride - 2 Cin, ss_off)); pixel tiles are 8 x 32
WGRAD_ACT_CASES = [
    (2, 8, 16, 8, 32, 8, 1, 1, True, 0, (0, 0)),      # PACK (Cin <= 8); one workgroup walks both images: the affine cache is refreshed
    (3, 24, 13, 9, 37, 3, 1, 3, True, 30, (0, 0)),    # channels off the 16-blocks, ragged tiles in both directions, three images in one workgroup
    (2, 3, 20, 5, 9, 3, 1, 1, False, 3, (0, 0)),      # PACK with Cin = 3, one partial tile per image
    (2, 40, 8, 17, 33, 8, 2, 2, True, 3, (0, 0)),     # 12 tiles over 2 workgroups: each meets both images
    (2, 16, 16, 8, 32, 4, 5, 1, True, 0, (0, 0)),     # more workgroups than tiles: three write all-zero partials
    (2, 16, 8, 9, 33, 2, 3, 2, True, 3, (9, 5)),      # ss_stride = 2 Cin + 9, ss_off = 5
]


@functools.lru_cache(maxsize=None)
def wgrad_act_case(B, Cin, Cout, H, W, groups, a_nt, with_ss, off):
    g = torch.Generator().manual_seed(Cin * 1009 + Cout * 101 + H * W)
    rn = lambda *s: torch.randn(*s, generator=g)
    # every image has its own spread on top of the channel offsets, gamma / beta differ per channel, scale / shift per image and channel:
    # an affine left over from the previous image, or from another channel, is far outside the gate
    x = offset_input(rn, g, B, Cin, H * W, off) * (1.0 + torch.arange(B, dtype=torch.float32))[:, None, None]
    dy = rn(B, Cout, H, W)
    gamma, beta = 1 + 0.3 * rn(Cin), 1 + 0.2 * rn(Cin)          # beta ~ 1: SiLU of a padding pixel that went through the affine is ~0.7, not 0
    scale, shift = (0.3 * rn(B, Cin), 0.3 * rn(B, Cin)) if with_ss else (None, None)
    out = dict(x=x, dy=dy, gamma=gamma, beta=beta, scale=scale, shift=shift, stats=piece_stats(x, unequal_cuts(H * W, a_nt, g)))
    for key, dt in (("ref", torch.float64), ("yard", torch.float32)):
        cast = lambda t: None if t is None else t.to(dt)
        a = group_act(cast(x), cast(gamma), cast(beta), cast(scale), cast(shift), groups).reshape(B, Cin, H, W)
        w = torch.zeros(Cout, Cin, 3, 3, dtype=dt, requires_grad=True)
        b = torch.zeros(Cout, dtype=dt, requires_grad=True)
        F.conv2d(a, w, b, padding=1).backward(cast(dy))
        out[key] = dict(dw=w.grad, db=b.grad)
    return out


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", WGRAD_ACT_CASES, ids=lambda c: "x".join(map(str, c[:8])) + ("-ss" if c[8] else "") + f"-off{c[9]}" + ("-sslayout" if c[10] != (0, 0) else ""))
def test_conv_wgrad_fused_activation(backend, case):
    """mi_conv_wgrad with a_stats set (the raw Block input goes through GroupNorm -> scale / shift -> SiLU while the tiles are staged) against
    fp64 autograd of conv2d(SiLU(...)) w.r.t. its weight and bias, within the fp32 yardstick: the per-image affine cache when a workgroup
    crosses an image boundary, zero padding that stays zero after SiLU, the PACK form (Cin <= 8), statistics in several tiles, ss_off / ss_stride"""
    B, Cin, Cout, H, W, groups, nwg, a_nt, with_ss, off, (ss_pad, ss_off) = case
    dev = setup(backend)
    lib = L.lib()
    what = f"wgrad-act {backend} B{B} {Cin}->{Cout} {H}x{W} g{groups} nwg{nwg} nt{a_nt} off{off}" + (f" ss+{ss_pad}@{ss_off}" if with_ss else "")
    ref = wgrad_act_case(B, Cin, Cout, H, W, groups, a_nt, with_ss, off)
    keep = {k: ref[k].to(dev).contiguous() for k in ("x", "dy", "gamma", "beta", "stats")}
    if with_ss:
        keep["ss"] = ss_table(B, Cin, ref["scale"], ref["shift"], 2 * Cin + ss_pad, ss_off).to(dev)
    runs = []
    for _ in range(2):
        bufs = dict(partial=guarded((lib.mi_conv_wgrad_workspace(Cin, Cout, nwg),), torch.float32, dev), dw=guarded((Cout, Cin, 3, 3), torch.float32, dev),
                    db=guarded((Cout,), torch.float32, dev))
        p = L.MiConvWgradParams()
        p.B, p.Cin, p.Cout, p.H, p.W, p.nwg = B, Cin, Cout, H, W, nwg
        p.a, p.dy, p.a_stats, p.a_nt, p.gamma, p.beta, p.groups, p.eps = (keep["x"].data_ptr(), keep["dy"].data_ptr(), keep["stats"].data_ptr(), a_nt,
                                                                          keep["gamma"].data_ptr(), keep["beta"].data_ptr(), groups, EPS)
        if with_ss:
            p.ss, p.ss_stride, p.ss_off = keep["ss"].data_ptr(), 2 * Cin + ss_pad, ss_off
        for k, (_, view) in bufs.items():
            setattr(p, k, view.data_ptr())
        L.check(lib.mi_conv_wgrad(C.byref(p), L.current_stream()), "mi_conv_wgrad")
        out = {}
        for k, (flat, view) in bufs.items():
            flat = flat.cpu()
            assert canary_intact(flat), f"{what}: the elements after {k} were overwritten"
            out[k] = flat[:view.numel()].view(view.shape)
        runs.append(out)
    for k in ("dw", "db", "partial"):
        assert torch.equal(bits(runs[0][k]), bits(runs[1][k])), f"{what}: {k} differs between two runs"
    assert torch.isfinite(runs[0]["partial"]).all(), f"{what}: a partial block was not written"
    within_yardstick(f"{what} dw", runs[0]["dw"], ref["ref"]["dw"], ref["yard"]["dw"])
    within_yardstick(f"{what} db", runs[0]["db"], ref["ref"]["db"], ref["yard"]["db"])


@pytest.mark.parametrize("backend", BACKENDS)
def test_conv_wgrad_fused_activation_rejections(backend):
    """the fused form is refused without gamma or beta, with groups not dividing Cin and with a_nt = 0; nothing is written"""
    dev = setup(backend)
    lib = L.lib()
    B, Cin, Cout, H, W = 1, 8, 8, 8, 8
    src = torch.zeros(B * Cin * H * W, dtype=torch.float64, device=dev)
    flat, buf = guarded((lib.mi_conv_wgrad_workspace(Cin, Cout, 1) + Cout * Cin * 9,), torch.float32, dev)

    def params(**kw):
        p = L.MiConvWgradParams()
        p.B, p.Cin, p.Cout, p.H, p.W, p.nwg = B, Cin, Cout, H, W, 1
        p.a = p.dy = p.a_stats = p.gamma = p.beta = src.data_ptr()
        p.dw, p.partial = buf.data_ptr(), buf[Cout * Cin * 9:].data_ptr()
        p.a_nt, p.groups, p.eps = 1, 4, EPS
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    for bad in (dict(gamma=None), dict(beta=None), dict(groups=3), dict(groups=0), dict(a_nt=0)):
        assert lib.mi_conv_wgrad(C.byref(params(**bad)), L.current_stream()) == MI_ERR_INVALID, bad
    assert torch.isnan(buf).all() and canary_intact(flat.cpu())
    L.check(lib.mi_conv_wgrad(C.byref(params()), L.current_stream()), "mi_conv_wgrad, the accepted form of the refused calls")


# ---------------------------------------------------------------------------------------------------------------------------------
# D. the data-gradient conv (mi_conv_fwd on the adjoint pack) across gradient magnitudes

class GuardedTorch:
    """stands in for the ``torch`` name inside train_ops: ``empty`` / ``empty_like`` hand out guarded buffers (NaN-filled, canary behind), everything
    else is torch's own -- the buffers train_ops allocates for its launches are then checked like the ones the tests allocate themselves"""

    def __init__(self):
        self.made = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *shape, dtype=torch.float32, device=None):
        if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)):
            shape = tuple(shape[0])
        flat, view = guarded(tuple(int(s) for s in shape), dtype, device)
        self.made.append(flat)
        return view

    def empty_like(self, t):
        return self.empty(tuple(t.shape), dtype=t.dtype, device=t.device)

    def assert_canaries(self, what):
        assert self.made, f"{what}: no buffer went through the guard"
        for flat in self.made:
            assert canary_intact(flat.cpu()), f"{what}: the elements after a buffer of {flat.numel() - CANARY} {flat.dtype} elements were overwritten"
        self.made.clear()


# The domain (the header comment of mi_conv_params).  The row-paired kernels scale every image by 2^ka,
# ka = clamp(4 - e(m), -K, K) with K = 60 (rp_clamp_exp), m = 4 * rms of the image over all its channels and e(m) the exponent with m in
# [2^(e-1), 2^e) (conv_rp.hip: the narrow prologue and gn_coef_kernel).  Unclamped, -K <= 4 - e(m) <= K, i.e. m in [2^(3-K), 2^(K+4)), the
# scaled image has 4 * rms in [8, 16) whatever its magnitude: a power-of-two scaling is exact, so the fp16 hi|lo split (22 mantissa bits while
# the lo half is a normal fp16, |scaled x| >= 2^-3; an absolute step of 2^-25 below that) and with it the relative error are THE SAME at every
# rms in  [RMS_LO, RMS_HI) = [2^(1-K), 2^(K+2)) = [2^-59, 2^62) ~ [1.7e-18, 4.6e18).
RP_CLAMP = 60
RMS_LO, RMS_HI = 2.0 ** (1 - RP_CLAMP), 2.0 ** (RP_CLAMP + 2)

# (Cin, Cout, H, W) of the FORWARD conv: the data gradient maps Cout -> Cin channels
DGRAD_FAMILIES = [(8, 16, 8, 16),       # 16 -> 8: row-paired narrow
                  (64, 128, 8, 16),     # 128 -> 64: row-paired wide (gn_coef_kernel sets the exponents)
                  (32, 64, 8, 16),      # 64 -> 32: the largest shape of the row-paired narrow kernels
                  (3, 8, 8, 16),        # 8 -> 3: row-paired narrow, an output-channel octet filled by three
                  (8, 8, 9, 13)]        # W % 4 != 0: direct-conv family (fp32 products, no range scaling)
# name -> (per-image rms, per-channel factors 10^-(c % 8) on top, kind of image 1)
DGRAD_SCALES = {
    "1..1e-8": ((1.0, 1e-4, 1e-8), False, ""),
    "1e-2..1e-10": ((1e-2, 1e-6, 1e-10), False, ""),
    "per-channel": ((1.0, 1e-4, 1e-8), True, ""),
    "zero-image": ((1.0, 0.0, 1e-4), False, ""),
    "one-pixel": ((1.0, 1e-3, 1e-4), False, "pixel"),
    "low-end": ((4.0 * RMS_LO, 1.0, 2.0 ** -30), False, ""),          # a factor 4 inside each end of the domain
    "high-end": ((RMS_HI / 4.0, 1.0, 2.0 ** 30), False, ""),
}


@functools.lru_cache(maxsize=None)
def dgrad_case(Cin, Cout, H, W, scales, per_channel, kind):
    """the weight, dy with the per-image rms `scales` (exactly: every image is normalised first), the fp64 data gradient and the fp32 yardstick"""
    g = torch.Generator().manual_seed(Cin * 131 + Cout * 17 + W)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * 0.2
    dy = torch.randn(len(scales), Cout, H, W, generator=g)
    if per_channel:
        dy = dy * (10.0 ** -(torch.arange(Cout) % 8).float())[None, :, None, None]
    if kind == "pixel":                     # the only non-zero of image 1 sits in a corner: its 3 x 3 footprint is cut by the padding
        dy[1] = 0.0
        dy[1, Cout // 2, H - 1, 0] = 1.7
    dy64 = dy.double()
    rms = (dy64 ** 2).mean((1, 2, 3), keepdim=True).sqrt()
    dy = (dy64 / rms * torch.tensor(scales, dtype=torch.float64)[:, None, None, None]).float()
    ref = F.conv_transpose2d(dy.double(), w.double(), padding=1)
    yard = F.conv_transpose2d(dy, w, padding=1)
    return dict(w=w, dy=dy, ref=ref, yard=yard)


def run_dgrad(dev, monkeypatch, case, stats_mode):
    """train_ops._conv3x3(dy, adjoint pack, None, stats=...) on guarded buffers; stats_mode None: mi_chan_stats_fwd, n: fp64 records of n row chunks"""
    guard = GuardedTorch()
    w = case["w"].to(dev)
    _, bwd = train_ops._packs(w)
    dy = case["dy"].to(dev).contiguous()
    B, Cc, H, W = dy.shape
    stats = None if stats_mode is None else chunk_stats(case["dy"].reshape(B, Cc, H * W), stats_mode).to(dev)
    monkeypatch.setattr(train_ops, "torch", guard)
    try:
        out = train_ops._conv3x3(dy, bwd, None, stats=stats)
    finally:
        monkeypatch.undo()
    out = out.cpu()
    guard.assert_canaries("data-gradient conv")
    return out


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("mode", [None, 1, 3], ids=["stats-kernel", "stats-1-chunk", "stats-3-chunks"])
@pytest.mark.parametrize("scales", list(DGRAD_SCALES))
@pytest.mark.parametrize("family", DGRAD_FAMILIES, ids=lambda f: "x".join(map(str, f)))
def test_dgrad_conv_across_magnitudes(backend, family, scales, mode, monkeypatch):
    """The data gradient of a 3x3 conv, _conv3x3(dy, adjoint pack), against fp64 conv_transpose2d on the CPU, per image: err < 2e-5 max |ref[b]|.
    Loss-weighted objectives (min-SNR) give per-image gradients orders of magnitude apart inside one batch; the row-paired kernels pick one fp16
    range exponent per image from its statistics, so every image must keep ITS OWN relative accuracy: rms 1 | 1e-4 | 1e-8 and 1e-2 | 1e-6 | 1e-10
    in one launch, channels a further 10^-(c % 8) apart, an all-zero image (exact zeros, everything finite) and an image with a single
    non-zero pixel.  The statistics come from mi_chan_stats_fwd (stats = None) and as fp64 records of 1 and 3 row chunks, as mi_block_bwd
    leaves them for its dx: all three must pass.
    "low-end" / "high-end": one image a factor 4 inside each end of the documented domain, rms in [2^-59, 2^62) (RMS_LO, RMS_HI above).
    Outside it -- measured with dgrad_outside() below, NOT asserted (16 -> 8 channels at 8 x 16, error / max |ref[b]| per image rms; emulator | MI355X):
        1e-18  5.5e-07 | 1.9e-07      1e-20  2.0e-06 | 2.0e-06      1e-22  1.6e-04 | 1.6e-04      1e-24  all zeros      1e-26  all zeros
    where fp32 torch holds 2e-7 .. 5e-7 throughout."""
    dev = setup(backend)
    sc, per_channel, kind = DGRAD_SCALES[scales]
    case = dgrad_case(*family, sc, per_channel, kind)
    what = f"dgrad {backend} {family[1]}->{family[0]} {family[2]}x{family[3]} {scales}"
    runs = [run_dgrad(dev, monkeypatch, case, mode) for _ in range(2)]
    assert torch.equal(bits(runs[0]), bits(runs[1])), f"{what}: two runs differ"
    conv_gate_per_image(f"{what} stats {'kernel' if mode is None else f'{mode} chunks'}", runs[0], case["ref"], case["yard"])


# Below RMS_LO the exponent stays at +60 and the scaled image shrinks: the absolute step 2^-25 of the lo half then weighs 2^-25 / (2^60 rms)
# of the image's rms -- 2e-6 of it at 1e-20, 1.6e-4 at 1e-22 (the table in the docstring above).  Below rms = 2^-75 ~ 2.6e-23 the mean square
# rounds to zero in fp32 ((float)(q / n) in the kernels' prologue), m = 0 selects "no scaling", and fp16 holds nothing of the image: all zeros.
# Above RMS_HI the exponent stays at -60 and the scaled image grows until an element passes the fp16 maximum (|x| >= 65504 * 2^60 ~ 7.5e22 -> inf).
DGRAD_OUTSIDE = (1e-18, 1e-20, 1e-22, 1e-24, 1e-26)


def dgrad_outside(dev, monkeypatch):
    """error / max |ref[b]| of the narrow row-paired data-gradient conv below its domain (a measurement for the table above, no assertion)"""
    case = dgrad_case(8, 16, 8, 16, DGRAD_OUTSIDE, False, "")
    out = run_dgrad(dev, monkeypatch, case, None)
    return [((out[b].double() - case["ref"][b]).abs().max() / case["ref"][b].abs().max()).item() for b in range(len(DGRAD_OUTSIDE))]


# ---------------------------------------------------------------------------------------------------------------------------------
# E. the hand-offs between two stacked Blocks

def make_blocks(c0, c1):
    torch.manual_seed(0)
    blocks = [Block(c0, c1, groups=8).train(), Block(c1, c0, groups=8).train()]
    with torch.no_grad():
        for blk in blocks:
            blk.groupnorm.weight.add_(0.3 * torch.randn(blk.groupnorm.weight.shape))
            blk.groupnorm.bias.add_(0.2 * torch.randn(blk.groupnorm.bias.shape))
    return blocks


def two_blocks_run(blocks, x, ss, gy, variant="", count=None):
    """y = block2(block1(x), ss) and every gradient; `count` (a list) receives the number of statistics passes after the forward and after the backward"""
    x = x.clone().requires_grad_()
    ss = tuple(t.clone().requires_grad_() for t in ss)
    for blk in blocks:
        blk.zero_grad(set_to_none=True)
    h = blocks[0](x)
    if variant == "inplace":
        h.mul_(1)                                          # written since its statistics were taken: the forward guard must drop them
    if variant == "hook":
        h.register_hook(lambda gr: gr.mul_(1))             # autograd hands block 1 the very dx of block 2, modified in place: the backward guard
    y = blocks[1](h, ss)
    if count is not None:
        count.append(count[0]())
    y.backward(gy)
    if count is not None:
        count.append(count[0]())
    out = dict(y=y.detach(), dx=x.grad, dscale=ss[0].grad, dshift=ss[1].grad)
    for i, blk in enumerate(blocks):
        out.update({f"b{i + 1}.dgamma": blk.groupnorm.weight.grad, f"b{i + 1}.dbeta": blk.groupnorm.bias.grad,
                    f"b{i + 1}.dw": blk.project.weight.grad, f"b{i + 1}.db": blk.project.bias.grad})
    return {k: v.detach().cpu().clone() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def two_blocks_case(c0, c1, H, W):
    blocks = make_blocks(c0, c1)
    g = torch.Generator().manual_seed(c0 + c1)
    B = 3
    x = torch.randn(B, c0, H, W, generator=g) * 1.5 + 0.2
    ss = tuple(torch.randn(B, c1, 1, 1, generator=g) * 0.3 for _ in range(2))
    gy = torch.randn(B, c0, H, W, generator=g) * 1e-3
    ref = two_blocks_run([copy.deepcopy(b).double() for b in blocks], x.double(), tuple(t.double() for t in ss), gy.double())
    yard = two_blocks_run(copy.deepcopy(blocks), x, ss, gy)             # host fp32 tensors without FORCE: the torch-op forms of the same modules
    return dict(blocks=blocks, x=x, ss=ss, gy=gy, ref=ref, yard=yard)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("variant", ["", "inplace", "hook"], ids=["handed-over", "inplace-forward", "hook-backward"])
@pytest.mark.parametrize("shape", [(8, 16, 16, 16), (64, 128, 8, 16)], ids=["8-16-8", "64-128-64"])
def test_two_blocks_hand_offs(backend, shape, variant, monkeypatch):
    """Block(c0 -> c1) then Block(c1 -> c0) with scale / shift through train_ops.block_forward, B = 3, against fp64 autograd of the same two modules
    on the CPU: y and dx within the per-image conv gate, every parameter gradient (last step mi_block_bwd or mi_conv_wgrad) within the yardstick.
    The statistics hand-offs are counted at train_ops._chan_stats: block 2's forward reads block 1's out_stats (ONE pass, for x) and block 1's
    backward reads block 2's dx_stats (ONE pass, for the outermost dy).  A record in the wrong slot would only move an fp16 range exponent,
    which no parity gate notices -- the count does.  "inplace-forward": h.mul_(1) between the blocks bumps h's version, the forward guard drops
    the record (two passes), and autograd then hands block 1 a new tensor (two passes).  "hook-backward": a gradient hook modifies block 2's dx
    in place, the `tag[1] == dy._version` guard of _BlockFn.backward drops its record (two passes in the backward, one in the forward).
    The results pass the same gates either way."""
    c0, c1, H, W = shape
    dev = setup(backend)
    what = f"two-blocks {backend} {c0}-{c1}-{c0} {H}x{W} {variant or 'handed-over'}"
    case = two_blocks_case(c0, c1, H, W)
    blocks = [copy.deepcopy(b).to(dev) for b in case["blocks"]]
    calls = []
    real = train_ops._chan_stats
    monkeypatch.setattr(train_ops, "_chan_stats", lambda t: (calls.append(tuple(t.shape)), real(t))[1])
    guard = GuardedTorch()
    monkeypatch.setattr(train_ops, "torch", guard)
    monkeypatch.setattr(train_ops, "FORCE", True)
    runs, counts = [], []
    for _ in range(2):
        calls.clear()
        count = [lambda: len(calls)]
        runs.append(two_blocks_run(blocks, case["x"].to(dev), tuple(t.to(dev) for t in case["ss"]), case["gy"].to(dev), variant, count))
        counts.append((count[1], count[2] - count[1]))
    monkeypatch.undo()
    guard.assert_canaries(what)
    print(f"{what}: statistics passes (forward, backward) {counts[0]}")
    assert counts[0] == counts[1] == {"": (1, 1), "inplace": (2, 2), "hook": (1, 2)}[variant], (what, counts)
    for k in runs[0]:
        assert torch.equal(bits(runs[0][k]), bits(runs[1][k])), f"{what}: {k} differs between two runs"
    ref, yard = case["ref"], case["yard"]
    for k in ("y", "dx"):
        conv_gate_per_image(f"{what} {k}", runs[0][k], ref[k], yard[k])
    for k in sorted(set(runs[0]) - {"y", "dx"}):
        within_yardstick(f"{what} {k}", runs[0][k], ref[k], yard[k])
