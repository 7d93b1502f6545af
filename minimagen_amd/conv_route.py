"""Which kernel, which tile, which flags: the launch policy of ``mi_conv_fwd`` in one place, for the engine's plans (``route``) and for the
training path's launches (``rp_code`` / ``direct_code``: the tile code only, no flags).  A leaf module: it knows the library's ``tile_cfg``
word (include/minimagen_hip.h) and nothing of the engine or the weights.  The tuning knobs stay ``engine``'s module globals; it hands their
current values in as a dict ``k`` keyed by ``KNOBS``."""
from __future__ import annotations

import ctypes as C
from typing import Callable, NamedTuple

from . import _lib as L

# flags of the tile_cfg word (mi_conv_params.tile_cfg)
MI_CONV_SPLIT16 = 0x100     # 16-channel outputs as two 8-channel workgroups
MI_CONV_REVERSE = 0x200     # row-paired path: workgroups take the images in reverse order (speed only)
MI_CONV_HALF = 0x400        # single fp16 term per product (the reduced-precision configuration)
MI_CONV_SPLIT8 = 0x800      # 8-channel outputs as two 4-channel workgroups
STRIPS_SHIFT, STRIPS_MASK = 12, 0xf         # bits 12..15: tiles (stripe kernel: statistics blocks) per workgroup, 0 = the library's choice
# tile codes (the low byte; mi_conv_tile_shape gives each one's output tile)
TILE_DIRECT_LARGE, TILE_DIRECT = 0, 2       # direct conv: images at least 64 wide above 64^2 / everything else
TILE_8X64, TILE_8X32 = 6, 7                 # row-paired matrix-core kernel (conv_rp.hip)
TILE_16X16 = 10                             # ... its wide k3 s1 member on images no wider than 16
TILE_GEMM = 11                              # wide GEMM kernel (conv_wide.hip): 8 x 16 pixels x 128 (or 64) channels per workgroup
TILE_STRIPE = 12                            # full-width row stripes (conv_stripe.hip)

DIRECT, NARROW, STRIPE, WIDE, GEMM = "direct", "narrow", "stripe", "wide", "gemm"      # kernel families
KNOBS = ("CONV_RP", "CONV_SPLIT8", "CONV_STRIPE", "CONV_REVERSE", "RP_NTILE", "RP_NTILE_BY", "RP_NTILE_PIPE", "ST_NBLK", "ST_NBLK_PIPE")


class Route(NamedTuple):
    family: str         # DIRECT | NARROW | STRIPE | WIDE | GEMM
    code: int           # tile code
    tiles: int          # statistics tiles per image (out_nt)
    reverse: bool       # the launch walks the image groups in reverse order: its consumer goes the other way
    word: int           # the complete tile_cfg word
    rp = property(lambda r: r.family != DIRECT)             # any matrix-core family: w_rp / res_w_rp fragments
    wide = property(lambda r: r.family in (WIDE, GEMM))     # wide regime: gn_coef / gn_exps buffers, mi_gn_coef_fwd ahead of the conv
    gemm = property(lambda r: r.family == GEMM)             # prepared operand planes, mi_conv_prep_fwd ahead of the conv, pack_conv_weight_ig fragments


def size_class(H: int, W: int) -> str:
    """the image-size classes of the per-class knobs: L > 128^2, M > 64^2, S smaller"""
    return "L" if H * W > 128 * 128 else ("M" if H * W > 64 * 64 else "S")


def tile_count(code: int, H: int, W: int) -> int:
    """tiles of the code's shape over an H x W image.  By image size ONLY: the per-tile partial statistics must reduce in the same order
    whatever the batch is, so that a sharded batch reproduces the unsharded rows bit for bit."""
    th, tw = C.c_int(), C.c_int()
    L.lib().mi_conv_tile_shape(code, C.byref(th), C.byref(tw))
    return -(-H // th.value) * -(-W // tw.value)


def tile_word(code: int, half: bool = False, split8: bool = False, reverse: bool = False, strips: int = 0) -> int:
    """the tile_cfg word of an engine launch (always with MI_CONV_SPLIT16)"""
    return code | MI_CONV_SPLIT16 | (MI_CONV_HALF if half else 0) | (MI_CONV_SPLIT8 if split8 else 0) | (MI_CONV_REVERSE if reverse else 0) \
        | ((strips & STRIPS_MASK) << STRIPS_SHIFT)


def reverse_order(k: dict, batch: int, producer_rev: bool) -> bool:
    """a row-paired conv walks the image groups in the opposite order of its producer: what was written last (still in the memory-side
    cache / L2) is read first (speed only; measured -1.2 % on the SR step)"""
    return bool(k["CONV_REVERSE"]) and batch % 8 == 0 and not producer_rev


def stripe_strips(k: dict, cls: str, tiles: int, batch: int, pipelined: bool, sr: bool) -> int:
    """statistics blocks per workgroup of the stripe kernel (must divide the blocks of an image; 0 = the library's choice)"""
    n, pipe = k["ST_NBLK"][cls], k["ST_NBLK_PIPE"][cls]
    if pipelined and pipe and tiles % pipe == 0 and batch * tiles // pipe >= 128 and sr:
        n = pipe        # (super-resolution U-Nets only: on the base U-Net it costs the base stage 7 %: 97.1 against 104.8 K steps/s, and gives the cascade nothing)
    return 0 if n and (tiles % n or n > 15) else n


def direct_code(H: int, W: int) -> int:
    """tile of the direct-conv family (and of the fp32 VALU CrossEmbed)"""
    return TILE_DIRECT_LARGE if (W >= 64 and H * W > 64 * 64) else TILE_DIRECT


def _rp_route(cin, cres, cout, H, W, stride, up2, wide_tiles):
    """-> (family, tile code) of the row-paired tile kernel.  Narrow layers (<= 64 in, <= 32 out: the BASELINE U-Nets) run the tuned
    single-kernel form; wider ones (Unet() default, Base, Super) the wide regime: output channels tiled over the grid, GroupNorm affine +
    operand exponents from a small per-image launch ahead of the conv"""
    if not (cin <= 64 and cres <= 64 and cout <= (16 if stride == 2 else (8 if up2 else 32))):
        if wide_tiles and stride == 1 and not up2 and cout >= 32 and (W % 64 == 0 or (W <= 16 and H > 8)):
            return WIDE, (TILE_8X64 if W % 64 == 0 else TILE_16X16)
        return WIDE, TILE_8X32
    if stride == 2 or up2:          # the down- / up-sampling members have one tile shape each
        return NARROW, (TILE_8X32 if stride == 2 else TILE_8X64)
    # four N tiles are only instantiated for the 8x32 tile.  Measured: 8x32 tiles for 8-channel layers at <= 64^2 (twice the workgroups) and for
    # images no wider than a tile; 16 output channels at 64^2 stay on 8x64 (B fragments staged per workgroup)
    return NARROW, (TILE_8X32 if cout > 16 or (H * W <= 64 * 64 and (W <= 32 or cout <= 8)) else TILE_8X64)


def rp_code(cin: int, cout: int, H: int, W: int):
    """-> (family, tile code) of a plain 3x3 stride-1 conv on the row-paired kernel, 8x32 tiles throughout the wide regime (the training path)"""
    return _rp_route(cin, 0, cout, H, W, stride=1, up2=False, wide_tiles=False)


def route(k: dict, *, batch: int, H: int, W: int, cin: int, cres: int, cout: int, ksize: int, stride: int, up2: bool, octets: bool, has_res: bool,
          frag_rp: bool, frag_ig: bool, half: bool, pipelined: bool, sr: bool, producer_rev: bool, stripe_rows: Callable[[], int]) -> Route:
    """The launch of one conv of a plan.  ``H`` / ``W``: of the OUTPUT; ``cin`` / ``cres``: channels of the (concatenated) input and of the
    input of a 1x1 residual conv (0: none or identity); ``octets``: all of those come in multiples of 8; ``has_res``: any residual;
    ``frag_rp`` / ``frag_ig``: row-paired / GEMM fragments exist for the weight and the residual weight; ``sr``: a super-resolution U-Net;
    ``stripe_rows``: mi_conv_stripe_rows on a probe of the launch, asked only for launches the stripe kernel's knob and family admit."""
    split8 = bool(k["CONV_SPLIT8"]) and H * W <= k["CONV_SPLIT8"] ** 2
    if not (k["CONV_RP"] and ((ksize == 3 and stride == 1) or (ksize == 4 and stride == 2 and not up2 and k["CONV_RP"] >= 2))
            and (not up2 or k["CONV_RP"] >= 2) and W % 4 == 0 and frag_rp and octets):
        code = direct_code(H, W)
        return Route(DIRECT, code, tile_count(code, H, W), False, tile_word(code, half, split8))
    cls = size_class(H, W)
    family, code = _rp_route(cin, cres, cout, H, W, stride, up2, wide_tiles=not half)
    rows = stripe_rows() if family == NARROW and not half and cls in k["CONV_STRIPE"] else 0
    if rows:
        family, code, tiles = STRIPE, TILE_STRIPE, H // rows
        strips = stripe_strips(k, cls, tiles, batch, pipelined, sr)
    else:
        if family == WIDE and ksize == 3 and stride == 1 and (not up2 or not has_res) and not half and cin % 32 == 0 and cres % 32 == 0 and cout % 64 == 0 and frag_ig:
            family, code = GEMM, TILE_GEMM
        tiles = tile_count(code, H, W)
        strips = k["RP_NTILE_BY"][cls] or k["RP_NTILE"]
        if not strips and pipelined and k["RP_NTILE_PIPE"][cls] and batch * tiles // k["RP_NTILE_PIPE"][cls] >= 256:
            strips = k["RP_NTILE_PIPE"][cls]    # (only while the launch still has a workgroup per CU: smaller batches keep the library's choice -- config 3 at B = 16: 39.1 K with, 40.7 K without)
    rev = reverse_order(k, batch, producer_rev)
    return Route(family, code, tiles, rev, tile_word(code, half, split8, rev, strips))

