"""Training on the device: the convolutions of ``Imagen.forward`` -> ``Unet.forward`` in train mode
(minimagen/Imagen.py:512-573, Unet.py:355-472) on the HIP kernels, forward AND backward.

``Block`` (GroupNorm -> [scale / shift] -> SiLU -> Conv3x3, layers.py:107-145) and the plain 3x3 convolutions (``final_conv``, the conv of
``Upsample``) become ``torch.autograd.Function``s:

* forward: ONE ``mi_conv_fwd`` launch -- the fused inference kernel (GroupNorm-apply + scale/shift + SiLU + conv, conv_rp.hip); only the
  block's INPUT is kept for the backward (the normalised / activated tensors are never stored: a third of the activation memory of the
  torch-op graph);
* backward, data gradient: the same kernel on the transposed, flipped weights (a 3x3 stride-1 convolution's adjoint is a 3x3 stride-1
  convolution), range-scaled by the gradient's own channel statistics;
* backward, weight / bias gradient: ``mi_conv_wgrad`` (conv_wgrad.hip: split-K fp32 matrix-core GEMM, deterministic);
* backward, pointwise part: ``mi_block_bwd`` (train_bwd.hip) -- GroupNorm / scale-shift / SiLU backward with the activation recomputed in
  registers from the saved input (row sums, apply, parameter gradients: three launches); the weight-gradient kernel applies the same
  activation while it stages its operand tiles, so the activated tensor is never written to memory in either direction.

Weights are re-packed into matrix-core fragments (``mi_pack_conv3``: one launch per weight and direction) when their version counter changes,
i.e. once per optimiser step; the exponents of all layers come back with one host round trip (``begin_step``).  The packs and everything else
derived from the weights are kept in two weak side tables (``_WeightState`` per weight tensor, ``_StepState`` per module), never on the
parameters or modules: copies and pickles of a module carry none of it.  ``CrossEmbedLayer``: matrix-core forward + ``mi_crossembed_wgrad``.
``CrossAttention`` (C < dim_head): the sampler's fold with the core on ``mi_folded_attn_fwd`` /
``mi_folded_attn_bwd`` (no score tensor, layers.CrossAttention._forward_folded).  The wide presets' attention layers (dim_head 64: the
multi-query ``Attention`` and the unfolded ``CrossAttention``, C >= dim_head): the projections, null row and LayerNorms as before, the core on
``flash_attention`` -- ``mi_flash_attn_train_fwd`` (the sampler's flash kernel, which also saves the logsumexp) and ``mi_flash_attn_train_bwd``
(FlashAttention-2 dq and dk / dv kernels, deterministic): no [heads x tokens x context] score tensor, forward or backward
(MINIMAGEN_FLASH_TRAIN=0: torch ops).  Conditioning and the remaining elementwise work stay on torch ops.  ``gradient all-reduce``: minimagen_amd/distributed.py::allreduce_gradients.
MINIMAGEN_TRAIN_HIP=0 switches the whole thing off (torch ops only)."""
from __future__ import annotations

import ctypes as C
import math
import os
import weakref

import numpy as np
import torch
import torch.nn.functional as F
from torch.utils.weak import WeakIdKeyDictionary

from . import _lib as L
from . import conv_route
from . import packing as P

ENABLED = os.environ.get("MINIMAGEN_TRAIN_HIP", "1") != "0"
FORCE = False                   # tests: take the HIP path for host tensors too (emulator build of the kernels)
WGRAD_NWG = 1024         # workgroups of a conv weight-gradient launch (split-K partials are added in a fixed order)
CE_WGRAD_NWG = int(os.environ.get("MINIMAGEN_CE_WGRAD_NWG", "512"))      # workgroups of the CrossEmbed weight-gradient launch


FINGERPRINT_EVERY = int(os.environ.get("MINIMAGEN_TRAIN_FINGERPRINT", "1"))     # content fingerprint of the conv weights every N-th training step (begin_step)
# weights on the GPU: begin_step re-packs EVERY conv weight from its current values on the device and takes the power-of-two fragment scaling
# from the maxima that the PREVIOUS step sent to the host (an asynchronous copy, a whole step old when it is read) -- no host round trip per
# step.  0 = the synchronous fingerprint path above (also what host tensors / the emulator take)
LAGGED = os.environ.get("MINIMAGEN_TRAIN_LAGGED_SCALES", "1") != "0"


def active(x: torch.Tensor) -> bool:
    """the HIP training path runs for fp32 GPU tensors under autograd (and for host tensors when a test forces the emulator)"""
    return ENABLED and x.dtype == torch.float32 and x.dim() == 4 and (x.is_cuda or FORCE)


class _Pack:
    """one conv weight (or its adjoint) in the layouts mi_conv_fwd reads: [Cin][3][3][Cout_pad] fp32 (direct-conv family) and the row-paired
    fp16 hi|lo fragments + their exponent -- written by ONE launch of mi_pack_conv3 on the device"""
    __slots__ = ("generic", "frag", "exp", "cout", "cin", "rp")

    def __init__(self, w: torch.Tensor, exp: int, adjoint: bool, launch: bool = True):
        lib = L.lib()
        Cout, Cin = w.shape[0], w.shape[1]
        self.cout, self.cin = (Cin, Cout) if adjoint else (Cout, Cin)
        ct = lib.mi_conv_cout_tile(self.cout)
        pad = -(-self.cout // ct) * ct
        self.generic = torch.empty(lib.mi_pack_conv3_floats(Cout, Cin, int(adjoint), pad, 1), dtype=torch.float32, device=w.device)
        self.frag = torch.empty(lib.mi_pack_conv3_floats(Cout, Cin, int(adjoint), pad, 0), dtype=torch.float16, device=w.device)
        self.exp, self.rp = exp, self.cin % 8 == 0
        if launch:                # (launch=False: the buffers only -- begin_step's lagged mode fills every pack of a U-Net with ONE mi_pack_conv3_multi)
            L.check(lib.mi_pack_conv3(w.data_ptr(), Cout, Cin, int(adjoint), exp, self.frag.data_ptr(), self.generic.data_ptr(), pad, L.current_stream()),
                    "mi_pack_conv3")

    def desc(self, w: torch.Tensor, adjoint: bool):
        """this pack's row of mi_pack_conv3_multi's descriptor table"""
        return (w.data_ptr(), self.frag.data_ptr(), self.generic.data_ptr(), w.shape[0], w.shape[1], int(adjoint), self.exp,
                self.generic.numel() // (self.cin * 9), 0)


def _pack_key(weight: torch.Tensor):
    """identity of the values a pack was made from: in-place updates bump the version counter (every torch optimiser), ``p.data = t`` and
    ``.to()`` change the storage pointer / device"""
    return (weight._version, weight.data_ptr(), str(weight.device))


class _WeightState:
    """what the training path derived from the values of one conv weight tensor"""
    __slots__ = ("key", "fwd", "bwd", "max_abs", "mark", "pattern")

    def __init__(self):
        self.key = self.fwd = self.bwd = None       # _pack_key the forward / adjoint packs were made at (None: no packs)
        self.max_abs = None                         # max |w| as begin_step last brought it to the host: the fragment scaling (_weight_exp, _ce_tables)
        self.mark = None                            # "values changed" compares this: the content fingerprint (synchronous mode) | the step number (lagged mode)
        self.pattern = None                         # the fingerprint's fixed pseudo-random pattern

    def renew(self, max_abs, mark):
        """the values changed: a new scale and mark, and everything derived from the old values goes"""
        self.max_abs, self.mark = max_abs, mark
        self.key = self.fwd = self.bwd = None

    def stale(self, w: torch.Tensor) -> bool:
        return self.fwd is None or self.key != _pack_key(w)


class _StepState:
    """what ``begin_step`` keeps between the steps of one module (and ``crossembed_forward`` between those of one CrossEmbed layer)"""
    __slots__ = ("counter", "sig", "dev", "k", "events", "host", "packs", "desc_key", "desc_dev", "ce_key", "ce_tables", "ce_index", "time_blocks")

    def __init__(self, sig=None, dev=None):
        self.counter = -1                                           # steps begun in the synchronous mode
        self.sig, self.dev, self.k = sig, dev, 0                    # lagged mode: ids of the conv weights, their device, slot counter
        self.events, self.host = [None, None], None                 # ... the two pinned buffers of maxima and the event behind each one's copy
        self.packs, self.desc_key, self.desc_dev = {}, None, None   # ... id(w) -> pack buffers; the rows of the descriptor table and its device copy
        self.ce_key, self.ce_tables, self.ce_index = None, None, {}     # CrossEmbed: what the Toeplitz tables were made from, the tables, the gather indices
        self.time_blocks = None                                     # Unet._forward_train: weak references to the ResnetBlocks of the stacked time MLP


# The side tables.  Keys are held weakly (tensors by identity), so an entry dies with its tensor / module; NO VALUE may hold a strong reference
# to its key or to any parameter (ids and data pointers instead), or nothing would ever be collected.  Nothing derived is kept on the
# parameters or modules themselves: copies and pickles of a module carry none of it.
_WEIGHTS = WeakIdKeyDictionary()                    # conv weight tensor -> _WeightState
_STEPS = weakref.WeakKeyDictionary()                # module -> _StepState
weight_state, step_state = _WEIGHTS.get, _STEPS.get                 # for tests and tools: the record of a weight tensor / a module, or None


def _packs(weight: torch.Tensor, exp=None):
    """(forward pack, data-gradient pack) of a [Cout][Cin][3][3] weight, kept in its _WeightState until it is updated in place"""
    st = _WEIGHTS.setdefault(weight, _WeightState())
    if not st.stale(weight):
        return st.fwd, st.bwd
    w = weight.detach()
    if exp is None:
        exp = P.rp_weight_exponent(float(w.abs().max()))
    w = w.contiguous()
    L.require_device(w)
    fwd = _Pack(w, exp, False)
    bwd = _Pack(w, exp, True)             # adjoint: W'[ci][co][ky][kx] = W[co][ci][2-ky][2-kx]
    st.key, st.fwd, st.bwd = _pack_key(weight), fwd, bwd
    return fwd, bwd


def begin_step(module: torch.nn.Module):
    """Once per training step.  Weights on the GPU (default): ``_begin_step_lagged`` -- every pack rebuilt from the current values by ONE launch, the
    fragment scaling from the previous step's asynchronously copied maxima, no host / GPU synchronisation.  Host tensors (the emulator) and
    MINIMAGEN_TRAIN_LAGGED_SCALES=0: re-pack every conv weight under ``module`` whose VALUES changed.  The version counter and the storage pointer
    (``_pack_key``) miss updates made through ``p.data`` (EMA copy-in, ``.data.mul_`` / ``.data.copy_``, hand-written SGD, an optimiser step
    replayed from a captured graph), so every weight also carries a content fingerprint (max |w|, ||w||_2): two fused multi-tensor launches
    and ONE device -> host copy for all layers -- the same copy that brings the exponents of the weights that need a new pack."""
    convs = [m for m in module.modules() if isinstance(m, torch.nn.Conv2d) and m.weight.is_floating_point()]
    if not convs:
        return
    ws = [m.weight for m in convs]
    if LAGGED and all(w.is_cuda for w in ws):
        return _begin_step_lagged(module, convs, ws)
    # The device -> host copy waits for the work queued before it (measured: 17.8 instead of 15.4 ms per SR step at B = 32, the host no longer
    # runs ahead of the GPU).  MINIMAGEN_TRAIN_FINGERPRINT=N checks every N-th step (0: never -- identity key only, round 3's behaviour);
    # weights whose identity key changed are always re-packed.
    step = _STEPS.setdefault(module, _StepState())
    step.counter += 1
    sts = [_WEIGHTS.setdefault(w, _WeightState()) for w in ws]
    stale_id = any(st.stale(w) for m, w, st in zip(convs, ws, sts) if m.kernel_size == (3, 3) and m.stride == (1, 1))
    check = FINGERPRINT_EVERY > 0 and step.counter % FINGERPRINT_EVERY == 0
    fp = None
    if check or stale_id:
        with torch.no_grad():
            det = [w.detach() for w in ws]
            # (max |w|, ||w||_2, ||w + r||_2) with r a fixed pseudo-random pattern per weight: the third term moves when values change sign or
            # place with both norms kept (w.data.neg_(), a channel permutation, an EMA copy of equal norm)
            for w, st in zip(ws, sts):
                if st.pattern is None or st.pattern.shape != w.shape or st.pattern.device != w.device:
                    g = torch.Generator().manual_seed(w.numel() * 2654435761 % (2 ** 31))
                    st.pattern = (torch.rand(w.shape, generator=g) - 0.5).to(w.device)
            pats = [st.pattern for st in sts]
            fp = torch.stack(torch._foreach_norm(det, float("inf")) + torch._foreach_norm(det, 2) + torch._foreach_norm(torch._foreach_add(det, pats), 2)).tolist()
    n = len(ws)
    for k, (m, w, st) in enumerate(zip(convs, ws, sts)):
        if fp is None:
            break
        mark = (fp[k], fp[n + k], fp[2 * n + k])
        if st.mark != mark:               # values changed behind the version counter
            st.renew(fp[k], mark)
        if m.kernel_size == (3, 3) and m.stride == (1, 1) and st.stale(w):
            with torch.no_grad():
                _packs(w, P.rp_weight_exponent(fp[k]))


_DESC_DTYPE = np.dtype([("w", "u8"), ("frag", "u8"), ("generic", "u8"), ("Cout", "i4"), ("Cin", "i4"), ("adjoint", "i4"), ("exp", "i4"),
                        ("cout_pad", "i4"), ("reserved", "i4")])          # mi_pack_conv3_desc


def _begin_step_lagged(module, convs, ws):
    """begin_step without a host round trip.  Every pack is rebuilt from the weights' CURRENT values (so no update can be missed, whichever way
    it was made); what comes from the host is only the exponent of the fragment scaling, and that tolerates stale maxima: a scale taken from the
    previous step's max |w| leaves 2^8 of head room to the fp16 range (max |w'| in [128, 256) against 65504), far more than an optimiser step
    moves a weight.  Per step: one fused max launch + one asynchronous copy into pinned memory, read at the NEXT call -- by then the copy is a
    whole step old, so the host keeps running ahead of the GPU.  The first call (no history) waits for its own maxima, once."""
    st = _STEPS.get(module)
    sig = tuple(id(w) for w in ws)
    if st is None or st.sig != sig or st.dev != ws[0].device:
        st = _STEPS[module] = _StepState(sig, ws[0].device)
        st.host = [torch.zeros(len(ws), dtype=torch.float32).pin_memory() for _ in range(2)]
    slot = st.k & 1
    with torch.no_grad():
        mx = torch.stack(torch._foreach_norm([w.detach() for w in ws], float("inf")))
        known = None
        if st.events[1 - slot] is not None:
            st.events[1 - slot].synchronize()
            known = st.host[1 - slot].tolist()
        st.host[slot].copy_(mx, non_blocking=True)
        ev = st.events[slot] = torch.cuda.Event()
        ev.record()
        if known is None or not all(math.isfinite(v) for v in known):
            ev.synchronize()
            known = st.host[slot].tolist()
        st.k += 1
        rows = []
        for m, w, mxk in zip(convs, ws, known):
            ws_ = _WEIGHTS.setdefault(w, _WeightState())
            ws_.renew(mxk, st.k)                               # _weight_exp / _ce_tables: the scale, and a mark that is new every step
            if m.kernel_size == (3, 3) and m.stride == (1, 1):
                exp = P.rp_weight_exponent(mxk)
                if not w.is_contiguous():
                    _packs(w, exp)
                    continue
                # the pack buffers live as long as the parameter keeps its storage: the descriptor table then only changes when an exponent does
                pk = st.packs.get(id(w))
                if pk is None or pk[0] != (w.data_ptr(), tuple(w.shape)):
                    wd = w.detach()
                    pk = st.packs[id(w)] = ((w.data_ptr(), tuple(w.shape)), _Pack(wd, exp, False, launch=False), _Pack(wd, exp, True, launch=False))
                pk[1].exp = pk[2].exp = exp
                rows += [pk[1].desc(w, False), pk[2].desc(w, True)]
                ws_.key, ws_.fwd, ws_.bwd = _pack_key(w), pk[1], pk[2]
        if rows:
            key = tuple(rows)
            if st.desc_key != key:                             # (first step, or an exponent moved: a small asynchronous upload through pinned memory)
                arr = np.array(rows, dtype=_DESC_DTYPE)
                host = torch.from_numpy(arr.view(np.uint8).reshape(-1)).pin_memory()
                if st.desc_dev is None or st.desc_dev.numel() != host.numel():
                    st.desc_dev = torch.empty(host.numel(), dtype=torch.uint8, device=ws[0].device)
                st.desc_dev.copy_(host, non_blocking=True)
                st.desc_key = key
            L.require_device(ws[0])
            L.check(L.lib().mi_pack_conv3_multi(st.desc_dev.data_ptr(), len(rows), 16, L.current_stream()), "mi_pack_conv3_multi")


def invalidate(module: torch.nn.Module):
    """Drop every pack / table derived from the parameters under ``module`` (they are rebuilt on the next use).  ``begin_step`` notices
    changed values by itself; this is for callers that replace parameters outside a training step (``load_state_dict``, ``_apply``)."""
    for m in module.modules():
        _STEPS.pop(m, None)
    for prm in module.parameters():
        _WEIGHTS.pop(prm, None)


def _chan_stats(x: torch.Tensor) -> torch.Tensor:
    """per-(image, channel) sum and sum of squares, [B][C][1][2] (one statistics tile): what a producing kernel's epilogue would have left"""
    B, Cc, H, W = x.shape
    st = torch.empty(B, Cc, 1, 2, dtype=torch.float64, device=x.device)
    L.check(L.lib().mi_chan_stats_fwd(x.data_ptr(), st.data_ptr(), B * Cc, H * W, L.current_stream()), "mi_chan_stats_fwd")
    return st


def _tag_stats(t: torch.Tensor, stats: torch.Tensor):
    """leave the channel statistics a kernel's epilogue wrote for ``t`` on the tensor itself: the only channel to its consumer that autograd
    offers (the next Block's forward; the previous Block's backward, which receives this very tensor as its output gradient)"""
    t._mi_stats = (stats, t._version)


def _tagged_stats(t: torch.Tensor):
    """the statistics left on ``t``: valid for this very tensor object while it has not been written since (else None: one statistics pass)"""
    stats, version = getattr(t, "_mi_stats", (None, None))
    return stats if (stats is not None and version == t._version and t.is_contiguous() and stats.shape[:2] == t.shape[:2]) else None


_ZEROS = {}


def _zero_bias(n: int, dev) -> torch.Tensor:
    key = (n, str(dev))
    if key not in _ZEROS:
        _ZEROS[key] = torch.zeros(n, dtype=torch.float32, device=dev)
    return _ZEROS[key]


def _conv3x3(x: torch.Tensor, pack: _Pack, bias, gn=None, ss=None, stats=None, want_stats: bool = False, res=None):
    """one mi_conv_fwd launch: out = conv3x3(act(x)) + bias with act = SiLU(GroupNorm(x) * (scale + 1) + shift) when ``gn`` is given"""
    lib = L.lib()
    B, Cin, H, W = x.shape
    Cout = pack.cout
    assert Cin == pack.cin
    L.require_device(x)
    out = torch.empty(B, Cout, H, W, dtype=torch.float32, device=x.device)
    if stats is None:
        stats = _chan_stats(x)
    if bias is None:
        bias = _zero_bias(Cout, x.device)
    keep = [stats, bias, out]
    p = L.MiConvParams()
    p.B, p.H, p.W = B, H, W
    p.in0 = L.MiAct(x.data_ptr(), Cin, stats.data_ptr(), stats.shape[2], 1.0, 0, 0)
    p.Cout, p.ksize, p.stride, p.up2 = Cout, 3, 1, 0
    p.w, p.bias, p.out = pack.generic.data_ptr(), bias.data_ptr(), out.data_ptr()
    if gn is not None:
        gamma, beta, groups, eps = gn
        p.gn_groups, p.gn_gamma, p.gn_beta, p.gn_eps = groups, gamma.data_ptr(), beta.data_ptr(), eps
        if ss is not None:
            p.scale_shift, p.ss_stride, p.ss_off = ss.data_ptr(), ss.shape[1], 0
    rp = pack.rp and W % 4 == 0
    if res is not None:             # identity residual added in the epilogue (row-paired narrow family only: residual_fusable); out_stats describe the SUM
        assert rp and Cin <= 64 and Cout <= 32 and res.shape == out.shape and res.is_contiguous()
        p.res0 = L.MiAct(res.data_ptr(), Cout, 0, 0, 1.0, 0, 0)
        keep.append(res)
    if rp:
        family, cfg = conv_route.rp_code(Cin, Cout, H, W)
        wide = family == conv_route.WIDE
        p.w_rp, p.w_rp_exp = pack.frag.data_ptr(), pack.exp
        if wide:
            coef = torch.empty(B, Cin, 4, dtype=torch.float32, device=x.device)
            exps = torch.empty(B, 2, dtype=torch.int32, device=x.device)
            keep += [coef, exps]
            p.gn_coef, p.gn_exps = coef.data_ptr(), exps.data_ptr()
        p.tile_cfg = cfg
        if wide:
            L.check(lib.mi_gn_coef_fwd(C.byref(p), L.current_stream()), "mi_gn_coef_fwd (training)")
    else:
        p.tile_cfg = conv_route.direct_code(H, W)
    out_stats = None
    if want_stats:                  # the epilogue's per-tile partial statistics of the OUTPUT: the next Block reads them instead of a statistics pass
        th, tw = C.c_int(), C.c_int()
        lib.mi_conv_tile_shape(p.tile_cfg & 0xff, C.byref(th), C.byref(tw))
        out_stats = torch.empty(B, Cout, (-(-H // th.value)) * (-(-W // tw.value)), 2, dtype=torch.float64, device=x.device)
        p.out_stats = out_stats.data_ptr()
    L.check(lib.mi_conv_fwd(C.byref(p), L.current_stream()), "mi_conv_fwd (training)")
    return (out, out_stats) if want_stats else out


def _wgrad(a: torch.Tensor, dy: torch.Tensor, want_bias: bool, act=None):
    """dW, db of a 3x3 conv from its input ``a`` and the output gradient; ``act`` = (stats, gamma, beta, groups, eps, ss): ``a`` is the raw
    Block input and the kernel applies GroupNorm -> scale/shift -> SiLU while staging the tiles"""
    lib = L.lib()
    B, Cin, H, W = a.shape
    Cout = dy.shape[1]
    tiles = B * (-(-H // 8)) * (-(-W // 32))
    nblk = (-(-Cin // 16)) * (-(-Cout // 16))
    nwg = max(1, min(tiles, max(64, WGRAD_NWG // nblk)))
    part = torch.empty(lib.mi_conv_wgrad_workspace(Cin, Cout, nwg), dtype=torch.float32, device=a.device)
    dw = torch.empty(Cout, Cin, 3, 3, dtype=torch.float32, device=a.device)
    db = torch.empty(Cout, dtype=torch.float32, device=a.device) if want_bias else None
    p = L.MiConvWgradParams()
    p.B, p.Cin, p.Cout, p.H, p.W = B, Cin, Cout, H, W
    p.a, p.dy, p.dw, p.db, p.partial, p.nwg = a.data_ptr(), dy.data_ptr(), dw.data_ptr(), L.ptr(db), part.data_ptr(), nwg
    if act is not None:
        stats, gamma, beta, groups, eps, ss = act
        p.a_stats, p.a_nt, p.gamma, p.beta, p.groups, p.eps = stats.data_ptr(), stats.shape[2], gamma.data_ptr(), beta.data_ptr(), groups, eps
        if ss is not None:
            p.ss, p.ss_stride, p.ss_off = ss.data_ptr(), ss.shape[1], 0
    L.check(lib.mi_conv_wgrad(C.byref(p), L.current_stream()), "mi_conv_wgrad")
    return dw, db


def _block_bwd(x, da, stats, gamma, beta, groups, eps, ss):
    """dx, dgamma, dbeta, d(scale|shift) of GroupNorm -> scale/shift -> SiLU from the activation's gradient (mi_block_bwd: three launches)"""
    lib = L.lib()
    B, Cc, H, W = x.shape
    HW = H * W
    nchunk = max(1, min(HW // 1024, -(-2048 // (B * Cc))))
    uv = torch.empty(B, Cc, nchunk, 2, dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x)
    dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(beta)
    dss = torch.empty(B, 2 * Cc, dtype=torch.float32, device=x.device) if ss is not None else None
    p = L.MiBlockBwdParams()
    p.B, p.C, p.HW, p.groups, p.nt, p.nchunk, p.eps = B, Cc, HW, groups, stats.shape[2], nchunk, eps
    p.x, p.da, p.x_stats, p.gamma, p.beta = x.data_ptr(), da.data_ptr(), stats.data_ptr(), gamma.data_ptr(), beta.data_ptr()
    if ss is not None:
        p.ss, p.ss_stride, p.ss_off = ss.data_ptr(), ss.shape[1], 0
    dx_stats = torch.empty(B, Cc, nchunk, 2, dtype=torch.float64, device=x.device)
    p.uv, p.dx, p.dgamma, p.dbeta, p.dss, p.dx_stats = uv.data_ptr(), dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), L.ptr(dss), dx_stats.data_ptr()
    L.check(lib.mi_block_bwd(C.byref(p), L.current_stream()), "mi_block_bwd")
    _tag_stats(dx, dx_stats)
    return dx, dgamma, dbeta, dss


class _BlockFn(torch.autograd.Function):
    """layers.py:131-145: fused HIP forward; backward = data-gradient conv (the forward kernel on the adjoint weights) -> mi_block_bwd
    (GroupNorm / scale-shift / SiLU backward, recomputing the activation in registers) + mi_conv_wgrad with the activation fused into its
    operand staging.  Saved for the backward: the block's input, its channel statistics and the scale|shift table -- nothing else."""

    @staticmethod
    def forward(ctx, x, gamma, beta, scale, shift, weight, bias, groups, eps, x_stats, residual=None):
        x = x.contiguous()
        fwd, _ = _packs(weight)
        g, b = gamma.detach().contiguous(), beta.detach().contiguous()
        ss = None
        if scale is not None:
            B = x.shape[0]
            ss = torch.cat((scale.detach().reshape(B, -1), shift.detach().reshape(B, -1)), 1).contiguous()
        stats = x_stats if x_stats is not None else _chan_stats(x)        # left by the producing Block's epilogue, or one statistics pass
        out, out_stats = _conv3x3(x, fwd, None if bias is None else bias.detach(), gn=(g, b, groups, eps), ss=ss, stats=stats, want_stats=True,
                                  res=None if residual is None else residual.detach())
        ctx.save_for_backward(x, g, b, ss, stats, weight)
        ctx.has_res = residual is not None
        ctx.groups, ctx.eps, ctx.has_bias, ctx.ss_shape = groups, eps, bias is not None, (None if scale is None else scale.shape)
        ctx.mark_non_differentiable(out_stats)
        return out, out_stats

    @staticmethod
    def backward(ctx, dy, _dstats=None):
        x, gamma, beta, ss, stats, weight = ctx.saved_tensors
        dy = dy.contiguous()
        _, bwd = _packs(weight)
        need = ctx.needs_input_grad
        dx = dgamma = dbeta = dscale = dshift = dw = db = None
        if any(need[:5]):
            da = _conv3x3(dy, bwd, None, stats=_tagged_stats(dy))         # left by the consumer Block's backward when dy is its dx, unmodified
            dx, dgamma, dbeta, dss = _block_bwd(x, da, stats, gamma, beta, ctx.groups, ctx.eps, ss)
            if dss is not None:
                Cc = x.shape[1]
                dscale, dshift = dss[:, :Cc].reshape(ctx.ss_shape), dss[:, Cc:].reshape(ctx.ss_shape)
        if need[5] or (ctx.has_bias and need[6]):
            dw, db = _wgrad(x, dy, ctx.has_bias and need[6], act=(stats, gamma, beta, ctx.groups, ctx.eps, ss))
        pick = lambda g, n: g if n else None
        return (pick(dx, need[0]), pick(dgamma, need[1]), pick(dbeta, need[2]), pick(dscale, need[3]), pick(dshift, need[4]),
                pick(dw, need[5]), db, None, None, None, (dy if (ctx.has_res and need[10]) else None))


class _ConvFn(torch.autograd.Function):
    """a plain 3x3 stride-1 convolution (Unet.py final_conv, layers.py:512-515 after the nearest x2): forward, data gradient and
    parameter gradients on the HIP kernels"""

    @staticmethod
    def forward(ctx, x, weight, bias, exp=None):
        x = x.contiguous()
        fwd, _ = _packs(weight, exp)
        out = _conv3x3(x, fwd, None if bias is None else bias.detach())
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        ctx.exp = exp
        return out

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy = dy.contiguous()
        _, bwd = _packs(weight, ctx.exp)
        need = ctx.needs_input_grad
        dx = _conv3x3(dy, bwd, None) if need[0] else None
        dw = db = None
        if need[1] or (ctx.has_bias and need[2]):
            dw, db = _wgrad(x, dy, ctx.has_bias and need[2])
        return dx, (dw if need[1] else None), db, None


def _ce_tables(layer, channels: int):
    """Toeplitz fragment tables of the matrix-core CrossEmbed kernel (packing.pack_crossembed_mfma), one per input half, kept in the layer's
    _StepState until any member conv is updated; ONE device->host copy of the (small) weights per optimiser step"""
    convs, st = layer.convs, _STEPS.setdefault(layer, _StepState())
    wst = [_WEIGHTS.get(c.weight) or _WeightState() for c in convs]
    key = tuple((_pack_key(c.weight), s.max_abs, s.mark) for c, s in zip(convs, wst))
    if st.ce_key == key:
        return st.ce_tables
    dev = convs[0].weight.device
    if LAGGED and dev.type == "cuda" and all(isinstance(s.mark, int) for s in wst):
        # begin_step's lagged mode: tables gathered on the device from the current weights, scaled by the exponents of the previous step's
        # whole-tensor maxima (>= the packed channel slice's own: the head room only grows) -- no device -> host copy
        idxs = st.ce_index
        exps = [P.rp_weight_exponent(s.max_abs) for s in wst]
        tabs = {}
        with torch.no_grad():
            for chan0 in range(0, convs[0].in_channels, channels):
                ik = (chan0, channels, tuple(tuple(c.weight.shape) for c in convs), str(dev))
                if ik not in idxs:
                    idxs[ik] = P.crossembed_mfma_gather_index([c.weight.shape for c in convs], chan0, channels).to(dev)
                tabs[chan0] = (P.pack_crossembed_mfma_device([c.weight for c in convs], idxs[ik], exps), exps)
        st.ce_key, st.ce_tables = key, tabs
        return tabs
    with torch.no_grad():
        flat = torch.cat([c.weight.detach().reshape(-1) for c in convs]).cpu()
    ws, off = [], 0
    for c in convs:
        n = c.weight.numel()
        ws.append(flat[off:off + n].reshape(c.weight.shape))
        off += n
    tabs = {}
    for chan0 in range(0, convs[0].in_channels, channels):
        tab, exps = P.pack_crossembed_mfma(ws, chan0, channels)
        tabs[chan0] = (tab.to(dev, non_blocking=True), exps)
    st.ce_key, st.ce_tables = key, tabs
    return tabs


def crossembed_supported(layer, x: torch.Tensor, lowres) -> bool:
    """the matrix-core forward + the shared-correlation weight gradient cover the reference's configuration: kernel sizes (3, 7, 15),
    dim_scales (4, 2, 2), stride 1, <= 4 image channels per half and <= 6 in total (mi_crossembed_wgrad), W % 4 == 0; the input must not need a gradient (it is the first layer)"""
    cv = layer.convs
    return (active(x) and layer.stride == 1 and [c.kernel_size[0] for c in cv] == [3, 7, 15] and [c.out_channels for c in cv] == [4, 2, 2]
            and x.shape[1] <= 4 and cv[0].in_channels <= 6 and x.shape[3] % 4 == 0 and not x.requires_grad and (lowres is None or (not lowres.requires_grad and lowres.shape == x.shape))
            and cv[0].in_channels == x.shape[1] * (2 if lowres is not None else 1) and all(c.bias is not None for c in cv))


class _CrossEmbedFn(torch.autograd.Function):
    """CrossEmbedLayer (layers.py:298-305) of the image (| low-res conditioning image): forward on the matrix-core Toeplitz kernel (one launch
    per input half, the second as addend of the first), weight / bias gradients by mi_crossembed_wgrad"""

    @staticmethod
    def forward(ctx, x, lowres, tabs, w0, b0, w1, b1, w2, b2):
        lib = L.lib()
        x = x.contiguous()
        B, Cc, H, W = x.shape
        ws_, bs_ = (w0, w1, w2), (b0, b1, b2)
        cfg = 8 if H * W >= 128 * 128 else 9
        out = torch.empty(B, 8, H, W, dtype=torch.float32, device=x.device)
        halves = [(x, 0)] + ([(lowres.contiguous(), Cc)] if lowres is not None else [])
        addend = None
        for src, chan0 in reversed(halves):             # the low-res half first (no bias), then the image half adds it and the biases
            dst = out if chan0 == 0 else torch.empty_like(out)
            p = L.MiCrossEmbedParams()
            p.B, p.H, p.W, p.in0, p.C0, p.n_kernels = B, H, W, src.data_ptr(), Cc, 3
            tab, exps = tabs[chan0]
            for i in range(3):
                p.ksize[i], p.cout[i], p.w_mfma_exp[i] = ws_[i].shape[-1], ws_[i].shape[0], exps[i]
                p.bias[i] = bs_[i].data_ptr() if chan0 == 0 else 0
            p.w_mfma, p.out, p.tile_cfg, p.addend = tab.data_ptr(), dst.data_ptr(), cfg, L.ptr(addend)
            L.check(lib.mi_crossembed_fwd(C.byref(p), L.current_stream()), "mi_crossembed_fwd (training)")
            addend = dst
        ctx.save_for_backward(x if lowres is None else torch.cat((x, lowres), 1))
        ctx.shapes = [w.shape for w in ws_]
        return out

    @staticmethod
    def backward(ctx, dy):
        lib = L.lib()
        (xin,) = ctx.saved_tensors
        dy = dy.contiguous()
        B, Cin, H, W = xin.shape
        tiles = B * (-(-H // 8)) * (-(-W // 32))
        nwg = max(1, min(tiles, CE_WGRAD_NWG))
        part = torch.empty(lib.mi_crossembed_wgrad_workspace(Cin, 15, nwg), dtype=torch.float32, device=xin.device)
        dws = [torch.empty(sh, dtype=torch.float32, device=xin.device) for sh in ctx.shapes]
        dbs = [torch.empty(sh[0], dtype=torch.float32, device=xin.device) for sh in ctx.shapes]
        p = L.MiCrossEmbedWgradParams()
        p.B, p.Cin, p.H, p.W, p.x, p.dy, p.n_kernels, p.partial, p.nwg = B, Cin, H, W, xin.data_ptr(), dy.data_ptr(), 3, part.data_ptr(), nwg
        for i in range(3):
            p.ksize[i], p.cout[i], p.dw[i], p.db[i] = ctx.shapes[i][-1], ctx.shapes[i][0], dws[i].data_ptr(), dbs[i].data_ptr()
        L.check(lib.mi_crossembed_wgrad(C.byref(p), L.current_stream()), "mi_crossembed_wgrad")
        return None, None, None, dws[0], dbs[0], dws[1], dbs[1], dws[2], dbs[2]


def crossembed_forward(layer, x: torch.Tensor, lowres) -> torch.Tensor:
    cv = layer.convs
    tabs = _ce_tables(layer, x.shape[1])
    return _CrossEmbedFn.apply(x, lowres, tabs, cv[0].weight, cv[0].bias, cv[1].weight, cv[1].bias, cv[2].weight, cv[2].bias)


def _aligned16(t: torch.Tensor) -> torch.Tensor:
    """a contiguous tensor whose first element is 16-byte aligned: ``t`` itself, or a copy when it is a view that starts in the middle of a line
    (the C = 16 attention kernels and the dim 8 / 16 / 32 LayerNorm kernels move 16 bytes at a time and refuse other pointers)"""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def folded_attention_supported(q: torch.Tensor, kf: torch.Tensor) -> bool:
    """mi_folded_attn_fwd / _bwd: fp32, C in {8, 16, 32}, J * C <= 6144 (the BASELINE U-Nets: C = 16, J = 259 / 261)"""
    return (ENABLED and q.dtype == torch.float32 and (q.is_cuda or FORCE) and q.shape[-1] in (8, 16, 32) and kf.shape[2] * kf.shape[3] <= 6144
            and kf.shape[2] <= 1024)


class _FoldedAttnFn(torch.autograd.Function):
    """out[b, i] = sum_h sum_j softmax_j(q[b, i] . kf[b, h, j]) vf[b, h, j] (the core of layers.CrossAttention._forward_folded) on the HIP
    kernels of attn_train.hip: the [tokens x heads x context] score tensor is never materialised, forward or backward; saved for the
    backward: q, kf, vf and the per-(token, head) logsumexp"""

    @staticmethod
    def forward(ctx, q, kf, vf, mask):
        lib = L.lib()
        q, kf, vf = _aligned16(q), _aligned16(kf), _aligned16(vf)
        L.require_device(q, kf, vf)
        B, n, Cc = q.shape
        H, J = kf.shape[1], kf.shape[2]
        m8 = None if mask is None else mask.to(torch.uint8).contiguous()
        out = torch.empty_like(q)
        lse = torch.empty(B, n, H, dtype=torch.float32, device=q.device)
        oh = torch.empty(B, n, H, Cc, dtype=torch.float32, device=q.device)       # per-head outputs (8 x the output: 67 MB at 64 x 64, B = 32)
        p = L.MiFoldedAttnParams()
        p.B, p.n, p.H, p.J, p.C, p.nchunk = B, n, H, J, Cc, 1
        p.q, p.kf, p.vf, p.mask, p.out, p.lse, p.oh = q.data_ptr(), kf.data_ptr(), vf.data_ptr(), L.ptr(m8), out.data_ptr(), lse.data_ptr(), oh.data_ptr()
        L.check(lib.mi_folded_attn_fwd(C.byref(p), L.current_stream()), "mi_folded_attn_fwd")
        ctx.save_for_backward(q, kf, vf, m8, lse, oh)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = L.lib()
        q, kf, vf, m8, lse, oh = ctx.saved_tensors
        dout = _aligned16(dout)
        B, n, Cc = q.shape
        H, J = kf.shape[1], kf.shape[2]
        nchunk = max(1, min(n // 128, -(-2048 // (B * H))))
        dq = torch.empty_like(q)
        dsum = torch.empty_like(lse)
        dkf = torch.empty(nchunk, B, H, J, Cc, dtype=torch.float32, device=q.device)
        dvf = torch.empty_like(dkf)
        p = L.MiFoldedAttnParams()
        p.B, p.n, p.H, p.J, p.C, p.nchunk = B, n, H, J, Cc, nchunk
        p.q, p.kf, p.vf, p.mask, p.lse = q.data_ptr(), kf.data_ptr(), vf.data_ptr(), L.ptr(m8), lse.data_ptr()
        p.dout, p.dsum, p.dq, p.dkf, p.dvf, p.oh = dout.data_ptr(), dsum.data_ptr(), dq.data_ptr(), dkf.data_ptr(), dvf.data_ptr(), oh.data_ptr()
        L.check(lib.mi_folded_attn_bwd(C.byref(p), L.current_stream()), "mi_folded_attn_bwd")
        return dq, (dkf[0] if nchunk == 1 else dkf.sum(0)), (dvf[0] if nchunk == 1 else dvf.sum(0)), None


def folded_attention(q: torch.Tensor, kf: torch.Tensor, vf: torch.Tensor, mask) -> torch.Tensor:
    return _FoldedAttnFn.apply(q, kf, vf, mask)


FLASH_TRAIN = os.environ.get("MINIMAGEN_FLASH_TRAIN", "1") != "0"      # 0: the wide attention layers' core on torch ops (A/B runs)


def flash_attention_supported(x: torch.Tensor, dim_head: int, attn_bias=None) -> bool:
    """mi_flash_attn_train_fwd / _bwd: fp32, dim_head 64, no additive attention bias (the multi-query Attention and the unfolded CrossAttention
    of Unet() default, Base and Super)"""
    return (ENABLED and FLASH_TRAIN and x.dtype == torch.float32 and (x.is_cuda or FORCE) and dim_head == 64 and attn_bias is None)


class _FlashAttnFn(torch.autograd.Function):
    """out[b, i, h] = softmax_j(scale * q[b, i, h] . k[b, j, kvh]) v[b, j, kvh] (q [B, n, H * 64] token-major, k / v [B, J, KVH * 64] with the
    null row and any context rows already in front, KVH = 1 or H) on the HIP kernels of attn_train_wide.hip: the [queries x context] score
    tensor is never materialised, forward or backward; saved for the backward: q, k, v, the output and the per-(query, head) logsumexp"""

    @staticmethod
    def forward(ctx, q, k, v, mask, scale):
        lib = L.lib()
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        L.require_device(q, k, v)
        B, n, inner = q.shape
        J = k.shape[1]
        m8 = None if mask is None else mask.to(torch.uint8).contiguous()
        out = torch.empty_like(q)
        lse = torch.empty(B, inner // 64, n, dtype=torch.float32, device=q.device)
        p = _flash_params(q, k, v, m8, out, lse, scale)
        work = torch.empty(lib.mi_flash_attn_train_workspace(B, n, p.heads, p.kv_heads, J, 0), dtype=torch.uint8, device=q.device)
        p.work, p.work_bytes = work.data_ptr(), work.numel()
        L.check(lib.mi_flash_attn_train_fwd(C.byref(p), L.current_stream()), "mi_flash_attn_train_fwd")
        ctx.save_for_backward(q, k, v, m8, out, lse)
        ctx.scale = scale
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = L.lib()
        q, k, v, m8, out, lse = ctx.saved_tensors
        dout = dout.contiguous()
        L.require_device(dout)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        p = _flash_params(q, k, v, m8, out, lse, ctx.scale)
        p.dout, p.dq, p.dk, p.dv = dout.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
        work = torch.empty(lib.mi_flash_attn_train_workspace(p.B, p.n, p.heads, p.kv_heads, p.J, 1), dtype=torch.uint8, device=q.device)
        p.work, p.work_bytes = work.data_ptr(), work.numel()
        L.check(lib.mi_flash_attn_train_bwd(C.byref(p), L.current_stream()), "mi_flash_attn_train_bwd")
        return dq, dk, dv, None, None


def _flash_params(q, k, v, m8, out, lse, scale):
    p = L.MiFlashAttnTrainParams()
    p.B, p.n, p.heads, p.kv_heads, p.J = q.shape[0], q.shape[1], q.shape[2] // 64, k.shape[2] // 64, k.shape[1]
    p.q, p.q_scale, p.k, p.v, p.mask = q.data_ptr(), scale * P.LOG2E, k.data_ptr(), v.data_ptr(), L.ptr(m8)
    p.out, p.lse = out.data_ptr(), lse.data_ptr()
    return p


def flash_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mask, scale: float) -> torch.Tensor:
    """softmax(scale * q k^T) v per head for dim_head 64: q [B, n, H * 64], k / v [B, J, KVH * 64] (KVH = 1: multi-query; KVH = H: a k / v
    head per head), mask [B, J] (False: the row takes no part) or None"""
    assert q.shape[-1] % 64 == 0 and k.shape[-1] in (64, q.shape[-1]) and v.shape == k.shape, (q.shape, k.shape, v.shape)
    return _FlashAttnFn.apply(q, k, v, mask, scale)


def layer_norm_supported(x: torch.Tensor, weight) -> bool:
    """mi_layernorm_fwd / _bwd: fp32, last dimension <= 1024, an affine weight"""
    return (ENABLED and torch.is_grad_enabled() and x.dtype == torch.float32 and (x.is_cuda or FORCE) and weight is not None and x.dim() >= 2
            and 0 < x.shape[-1] <= 1024 and x.numel() > 0)


class _LayerNormFn(torch.autograd.Function):
    """LayerNorm over the last dimension (the reference's LayerNorm, layers.py:333-343, and the nn.LayerNorm members of the conditioning stack) on
    train_ln.hip, forward and backward; saved for the backward: the input and (mean, rstd) per row -- not the normalised tensor"""

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        lib = L.lib()
        x2 = _aligned16(x).view(-1, x.shape[-1])
        L.require_device(x2)
        rows, dim = x2.shape
        y = torch.empty_like(x2)
        stat = torch.empty(rows, 2, dtype=torch.float32, device=x.device)
        w = weight.detach().contiguous()
        b = None if bias is None else bias.detach().contiguous()
        L.check(lib.mi_layernorm_fwd(x2.data_ptr(), w.data_ptr(), L.ptr(b), y.data_ptr(), stat.data_ptr(), rows, dim, float(eps), L.current_stream()), "mi_layernorm_fwd")
        ctx.save_for_backward(x2, w, stat)
        ctx.has_bias = bias is not None
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        lib = L.lib()
        x2, w, stat = ctx.saved_tensors
        rows, dim = x2.shape
        dy2 = _aligned16(dy).view(rows, dim)
        dx = torch.empty_like(x2)
        need_w = ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2])
        partial = dgamma = dbeta = None
        if need_w:
            partial = torch.empty(lib.mi_layernorm_bwd_nwg(rows, dim), 2, dim, dtype=torch.float32, device=x2.device)
            dgamma = torch.empty(dim, dtype=torch.float32, device=x2.device)
            dbeta = torch.empty(dim, dtype=torch.float32, device=x2.device) if ctx.has_bias else None
        L.check(lib.mi_layernorm_bwd(dy2.data_ptr(), x2.data_ptr(), w.data_ptr(), stat.data_ptr(), dx.data_ptr(), L.ptr(partial), L.ptr(dgamma), L.ptr(dbeta),
                                     rows, dim, L.current_stream()), "mi_layernorm_bwd")
        return dx.view(dy.shape), dgamma, dbeta, None


def layer_norm(x: torch.Tensor, weight, bias, eps: float = 1e-5) -> torch.Tensor:
    """``F.layer_norm(x, x.shape[-1:], weight, bias, eps)`` on the HIP kernels where they apply (training on the device), else torch's"""
    if layer_norm_supported(x, weight):
        return _LayerNormFn.apply(x, weight, bias, eps)
    return torch.nn.functional.layer_norm(x, x.shape[-1:], weight, bias, eps)


def residual_fusable(block, x: torch.Tensor, residual) -> bool:
    """the conv epilogue can add ``residual`` (ResnetBlock: h + res_conv(x), layers.py:439): narrow row-paired family, same shape, fp32, contiguous"""
    conv = block.project
    return (residual is not None and isinstance(block.groupnorm, torch.nn.GroupNorm) and conv.in_channels % 8 == 0 and x.shape[-1] % 4 == 0
            and conv.in_channels <= 64 and conv.out_channels <= 32 and residual.dtype == torch.float32 and residual.is_contiguous()
            and tuple(residual.shape) == (x.shape[0], conv.out_channels, x.shape[2], x.shape[3]))


def block_forward(block, x: torch.Tensor, scale_shift=None, residual=None) -> torch.Tensor:
    """``Block.forward`` (layers.py:131-145) through _BlockFn; ``residual`` (optional) is added to the output -- in the conv's epilogue where the
    kernel family allows (one launch and one statistics pass less per ResnetBlock: the next Block reads the statistics of the SUM)"""
    gnm = block.groupnorm
    conv = block.project
    scale, shift = scale_shift if scale_shift is not None else (None, None)
    if not isinstance(gnm, torch.nn.GroupNorm):             # Block(norm=False): not a layer of the reference's U-Nets; keep the semantics
        h = x if scale is None else x * (scale + 1) + shift
        out = _ConvFn.apply(F.silu(h), conv.weight, conv.bias)
        return out if residual is None else out + residual
    x_stats = _tagged_stats(x)      # handed over by the Block that produced x (block1 -> block2 of a ResnetBlock without cross-attention)
    fuse = residual_fusable(block, x, residual)
    out, out_stats = _BlockFn.apply(x, gnm.weight, gnm.bias, scale, shift, conv.weight, conv.bias, gnm.num_groups, gnm.eps, x_stats, residual if fuse else None)
    if residual is not None and not fuse:
        return out + residual
    _tag_stats(out, out_stats)
    return out


def conv3x3_forward(conv: torch.nn.Conv2d, x: torch.Tensor) -> torch.Tensor:
    return _ConvFn.apply(x, conv.weight, conv.bias)


def _weight_exp(weight: torch.Tensor):
    """exponent of the fragment scaling from the max |w| that begin_step() already brought to the host (None: _packs fetches it)"""
    st = _WEIGHTS.get(weight)
    return P.rp_weight_exponent(st.max_abs) if st is not None and st.max_abs is not None else None


def is_conv1x1(m, x=None) -> bool:
    ok = isinstance(m, torch.nn.Conv2d) and m.kernel_size == (1, 1) and m.stride == (1, 1) and m.padding == (0, 0) and m.groups == 1
    if ok and x is not None:
        ok = conv_shape_supported(m.in_channels, m.out_channels, x.shape[-1])
    return ok


def conv1x1_forward(conv: torch.nn.Conv2d, x: torch.Tensor) -> torch.Tensor:
    """A 1x1 convolution (ResnetBlock.res_conv, layers.py:415; Parallel's second member, :346-356) as the centre tap of a 3x3 one: forward, data
    gradient and weight gradient on the HIP 3x3 kernels (the zero taps cost matrix-core work on an 8..32-channel layer that is bound by its
    activation traffic); autograd takes the centre of the 3x3 weight gradient back to the parameter."""
    w3 = F.pad(conv.weight, (1, 1, 1, 1))
    return _ConvFn.apply(x, w3, conv.bias, _weight_exp(conv.weight))


def is_conv4x4s2(m, x=None) -> bool:
    ok = isinstance(m, torch.nn.Conv2d) and m.kernel_size == (4, 4) and m.stride == (2, 2) and m.padding == (1, 1) and m.groups == 1 \
        and m.dilation == (1, 1) and m.padding_mode == "zeros"
    if ok and x is not None:
        ok = x.shape[-1] % 2 == 0 and x.shape[-2] % 2 == 0 and conv_shape_supported(4 * m.in_channels, m.out_channels, x.shape[-1] // 2)
    return ok


def conv4x4s2_forward(conv: torch.nn.Conv2d, x: torch.Tensor) -> torch.Tensor:
    """Downsample (layers.py:308-319: Conv2d k4 s2 p1) as a 3x3 stride-1 convolution over the space-to-depth image: with x'[4c + 2py + px][Y][X] =
    x[c][2Y + py][2X + px] the tap ky of the stride-2 kernel reads row 2y + ky - 1 = 2 (y + a) + py, (a, py) = (-1, 1), (0, 0), (0, 1), (1, 0)
    for ky = 0..3 -- a 3x3 kernel over 4 Cin channels in which 20 of the 36 (a, py, b, px) combinations are zero.  pixel_unshuffle is one copy;
    forward, data gradient and weight gradient then run on the HIP 3x3 kernels, and autograd scatters / gathers between the two weight layouts
    (16 slices of a [Cout, Cin, 4, 4] tensor)."""
    w = conv.weight
    Cout, Cin = w.shape[0], w.shape[1]
    # ONE gather for the re-layout (and one index_add in its backward): 16 sliced assignments were ~50 small launches per Downsample and step
    # on a training step that is bound by its launch count
    w3 = F.pad(w.reshape(Cout, Cin, 16), (0, 1)).index_select(2, _k4_index(w.device)).reshape(Cout, 4 * Cin, 3, 3)
    return _ConvFn.apply(F.pixel_unshuffle(x, 2), w3, conv.bias, _weight_exp(w))


_K4_INDEX = {}


def _k4_index(dev) -> torch.Tensor:
    """[py, px, a + 1, b + 1] flattened -> 4 ky + kx of the stride-2 kernel's tap, 16 (a zero column appended to the taps) where there is none"""
    key = str(dev)
    if key not in _K4_INDEX:
        idx = torch.full((2, 2, 3, 3), 16, dtype=torch.long)
        tap = ((0, 1), (1, 0), (1, 1), (2, 0))                        # ky -> (a + 1, py)
        for ky in range(4):
            for kx in range(4):
                (ay, py), (ax, px) = tap[ky], tap[kx]
                idx[py, px, ay, ax] = 4 * ky + kx
        _K4_INDEX[key] = idx.reshape(-1).to(dev)
    return _K4_INDEX[key]


def conv_shape_supported(cin: int, cout: int, W: int, groups: int = 0) -> bool:
    """the limits of mi_conv_fwd / mi_conv_wgrad as the kernels check them: the row-paired matrix-core family needs channel octets and
    W % 4 == 0 and goes up to 4096 input channels (wide regime); everything else runs the direct-conv family (<= 256 input channels);
    GroupNorm with at most 32 groups.  Both directions must fit (the data gradient is the same conv with the channel counts swapped)."""
    def one(ci, co):
        rp = ci % 8 == 0 and W % 4 == 0
        return ci <= (4096 if rp else 256)
    return one(cin, cout) and one(cout, cin) and groups <= 32


def is_plain_conv3x3(m, x=None) -> bool:
    ok = isinstance(m, torch.nn.Conv2d) and m.kernel_size == (3, 3) and m.stride == (1, 1) and m.padding == (1, 1) and m.groups == 1 \
        and m.dilation == (1, 1) and m.padding_mode == "zeros"
    if ok and x is not None:
        ok = conv_shape_supported(m.in_channels, m.out_channels, x.shape[-1])
    return ok


def block_supported(block, x: torch.Tensor) -> bool:
    gnm = block.groupnorm
    groups = gnm.num_groups if isinstance(gnm, torch.nn.GroupNorm) else 0
    return conv_shape_supported(block.project.in_channels, block.project.out_channels, x.shape[-1], groups)


# ---- the front and the loss of a training step for the prediction objectives (csrc/objective.hip)
_TARGET_KINDS = {None: 0, 'noise': 0, 'v': 1, 'x_start': 2}           # MI_TARGET_*: the noise objective's target is the caller's noise tensor
_LOSS_KINDS = {'l1': 0, 'l2': 1, 'huber': 2}                            # MI_LOSS_*
_LOSS_FNS = {'l1': F.l1_loss, 'l2': F.mse_loss, 'huber': F.smooth_l1_loss}


def objective_active(x: torch.Tensor) -> bool:
    """mi_diffuse_fwd / mi_objective_loss_fwd run for fp32 GPU tensors (and for host tensors when a test forces the emulator), with or without
    autograd: the no-grad evaluation of the loss takes them too"""
    return ENABLED and x.dtype == torch.float32 and (x.is_cuda or FORCE)


def _diffuse_table(sched, dev) -> torch.Tensor:
    """[T][2] = (sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod): the fp32 values of the schedule's buffers, on ``dev``, built once"""
    tab = getattr(sched, "_diffuse_tab", None)
    if tab is None or tab.device != dev:
        tab = sched._diffuse_tab = torch.stack((sched.sqrt_alphas_cumprod, sched.sqrt_one_minus_alphas_cumprod), dim=1).to(dev).contiguous()
    return tab


def diffuse(x: torch.Tensor, noise: torch.Tensor, times: torch.Tensor, sched, *, normalize: bool, target=None):
    """-> (x_t, target): ``x`` [B, ...] normalised to [-1, 1] when ``normalize``, corrupted to the timesteps ``times`` (int64 [B]) of ``sched``
    with ``noise``, and what a U-Net that predicts ``target`` is compared with -- 'v': sqrt(abar) noise - sqrt(1 - abar) x0; 'x_start': the
    normalised x0; 'noise': ``noise`` itself; None: nothing (the low-resolution conditioning image).  One mi_diffuse_fwd launch where
    objective_active, the torch expressions of Imagen._p_losses otherwise: the same bits either way.  Not differentiable in ``x`` on the
    kernel (the training loss never needs that)."""
    if target not in _TARGET_KINDS:
        raise ValueError(f"target must be one of 'noise', 'x_start', 'v' or None, got {target!r}")
    if not objective_active(x):
        x0 = x * 2 - 1 if normalize else x
        x_t = sched.q_sample(x_start=x0, t=times, noise=noise)
        return x_t, {None: None, 'noise': noise, 'x_start': x0}[target] if target != 'v' else sched.calculate_v(x0, times, noise)
    xc, nc, tc = x.detach().contiguous(), noise.detach().contiguous(), times.contiguous()
    if tc.dtype != torch.int64 or tc.shape != (xc.shape[0],) or nc.shape != xc.shape:
        raise L.MinImagenHipError(f"diffuse: times must be int64 [{xc.shape[0]}] and noise shaped like x, got {tc.dtype} {tuple(tc.shape)}, {tuple(nc.shape)}")
    tab = _diffuse_table(sched, xc.device)
    L.require_device(xc, nc, tc, tab)
    kind = _TARGET_KINDS[target]
    x_t = torch.empty_like(xc)
    tgt = torch.empty_like(xc) if kind else None
    B = xc.shape[0]
    p = L.MiDiffuseParams(B, xc.numel() // B, tab.shape[0], 1 if normalize else 0, kind, xc.data_ptr(), nc.data_ptr(), tc.data_ptr(), tab.data_ptr(),
                          x_t.data_ptr(), L.ptr(tgt))
    L.check(L.lib().mi_diffuse_fwd(C.byref(p), L.current_stream()), "mi_diffuse_fwd")
    return x_t, (noise if target == 'noise' else tgt)


class _ObjectiveLossFn(torch.autograd.Function):
    """mi_objective_loss_fwd (+ its finish) and mi_objective_loss_bwd: the weighted loss as one fp32 on the device; when ``pred`` wants a
    gradient the forward pass also writes g = w l'(d) / (B n) (saved for the backward, which is one launch: g * grad_out)"""

    @staticmethod
    def forward(ctx, pred, target, times, weights, loss_type):
        lib = L.lib()
        pc, tg = pred.detach().contiguous(), target.detach().contiguous()
        tc = None if times is None else times.contiguous()
        L.require_device(pc, tg, tc, weights)
        B = pc.shape[0]
        n = pc.numel() // B
        dev = pc.device
        partials = torch.empty(B * lib.mi_objective_chunks(n), dtype=torch.float64, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        grad = torch.empty_like(pc) if ctx.needs_input_grad[0] else None          # (the no-grad evaluation has no gradient buffer)
        p = L.MiObjectiveLossParams(B, n, _LOSS_KINDS[loss_type], 0 if weights is None else weights.numel(), pc.data_ptr(), tg.data_ptr(), L.ptr(tc),
                                    L.ptr(weights), partials.data_ptr(), loss.data_ptr(), L.ptr(grad))
        L.check(lib.mi_objective_loss_fwd(C.byref(p), L.current_stream()), "mi_objective_loss_fwd")
        if grad is not None:
            ctx.save_for_backward(grad)
        return loss.view(())

    @staticmethod
    def backward(ctx, grad_out):
        (g,) = ctx.saved_tensors
        go = grad_out.detach().to(torch.float32).contiguous()
        L.require_device(go)
        dpred = torch.empty_like(g)
        L.check(L.lib().mi_objective_loss_bwd(g.data_ptr(), go.data_ptr(), dpred.data_ptr(), g.numel(), L.current_stream()), "mi_objective_loss_bwd")
        return dpred, None, None, None, None


def objective_loss(pred: torch.Tensor, target: torch.Tensor, times: torch.Tensor = None, weights: torch.Tensor = None, loss_type: str = 'l2') -> torch.Tensor:
    """(1 / (B n)) sum_b w[times[b]] sum_i l(pred - target) as a scalar tensor, l = 'l1' | 'l2' | 'huber' (smooth-l1, beta = 1) and ``weights`` an
    fp32 table [T] on the device of ``pred`` (GaussianDiffusion.loss_weight_table) or None for w = 1.  Differentiable in ``pred``.  On
    objective.hip where objective_active (sums in fp64, no host synchronisation), else the same mathematics in torch ops."""
    if loss_type not in _LOSS_KINDS:
        raise ValueError(f"loss_type must be one of {tuple(_LOSS_KINDS)}, got {loss_type!r}")
    if target.shape != pred.shape:
        raise ValueError(f"objective_loss: pred {tuple(pred.shape)} and target {tuple(target.shape)} differ in shape")
    if weights is not None and (times is None or times.dtype != torch.int64 or times.shape != (pred.shape[0],)):
        raise ValueError("objective_loss: weights need times, int64 [B]")
    if objective_active(pred):
        if weights is not None and (weights.dtype != torch.float32 or weights.dim() != 1):
            raise ValueError("objective_loss: weights must be float32 [T]")
        return _ObjectiveLossFn.apply(pred, target, times, None if weights is None else weights.contiguous(), loss_type)
    per = _LOSS_FNS[loss_type](pred, target, reduction='none').flatten(1).mean(dim=1)
    if weights is not None:
        per = per * weights[times]
    return per.mean()
