"""CrossEmbed micro-benchmark (dev tool): python tools/bench_ce.py [B H W cfg mfma half]  -- SR shape by default.
With mfma and fp32 it also times the pre-Downsample (k4 s2, 8 -> 8) that follows CrossEmbed in a memory_efficient U-Net, and the fused
launch (mi_init_down_fwd, both tile shapes) that replaces the pair."""
import ctypes as C
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from minimagen_amd import _lib as L
from minimagen_amd import packing as P

a = sys.argv[1:]
B, H, W = (int(a[0]), int(a[1]), int(a[2])) if len(a) >= 3 else (32, 256, 256)
cfg = int(a[3]) if len(a) > 3 else 8
mfma = (a[4] != "0") if len(a) > 4 else True
half = (a[5] != "0") if len(a) > 5 else False
dev = torch.device("cuda:0")
L.use_library(os.environ.get("MINIMAGEN_HIP_LIB", L.DEFAULT_LIB))
lib = L.lib()
g = torch.Generator().manual_seed(0)
x = torch.randn(B, 3, H, W, generator=g).to(dev)
ws = [torch.randn(co, 3, k, k, generator=g) * 0.1 for k, co in zip((3, 7, 15), (4, 2, 2))]
bs = [torch.randn(co, generator=g).to(dev) for co in (4, 2, 2)]
add = torch.randn(B, 8, H, W, generator=g).to(dev)
p = L.MiCrossEmbedParams()
p.B, p.H, p.W, p.in0, p.C0, p.n_kernels = B, H, W, x.data_ptr(), 3, 3
wp = [w.permute(1, 2, 3, 0).contiguous().to(dev) for w in ws]
tab, exps = P.pack_crossembed_mfma(ws, 0, 3)
tab = tab.to(dev)
for i, (k, co) in enumerate(zip((3, 7, 15), (4, 2, 2))):
    p.ksize[i], p.cout[i], p.w[i], p.bias[i], p.w_mfma_exp[i] = k, co, wp[i].data_ptr(), bs[i].data_ptr(), exps[i]
if mfma:
    p.w_mfma = tab.data_ptr()
th, tw = C.c_int(), C.c_int()
lib.mi_conv_tile_shape(cfg, C.byref(th), C.byref(tw))
nt = -(-H // th.value) * -(-W // tw.value)
out = torch.empty(B, 8, H, W, device=dev)
ost = torch.zeros(B, 8, nt, 2, dtype=torch.float64, device=dev)
p.out, p.out_stats, p.tile_cfg, p.addend = out.data_ptr(), ost.data_ptr(), cfg | (0x400 if half else 0), add.data_ptr()
st = L.current_stream()
for _ in range(3):
    L.check(lib.mi_crossembed_fwd(C.byref(p), st), "crossembed")
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(20):
    L.check(lib.mi_crossembed_fwd(C.byref(p), st), "crossembed")
e1.record(); torch.cuda.synchronize()
us = e0.elapsed_time(e1) / 20 * 1e3
print(f"crossembed B{B} {H}x{W} cfg {cfg} mfma={int(mfma)} half={int(half)}: {us:.1f} us")


def timed(fn, q, name, reps=20):
    for _ in range(3):
        L.check(fn(C.byref(q), st), name)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        L.check(fn(C.byref(q), st), name)
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


PHASES = ["issue loads", "wait + max + split + LDS write", "GEMM", "epilogue"]


def trace():
    """-DMI_TRACE build only: shader-clock time per phase of the first 1024 workgroups of the LAST launch, and their wall-clock starts / ends"""
    if not hasattr(lib, "mi_debug_read_trace_ce"):
        return
    import numpy as np
    buf = np.zeros(1024 * 8, dtype=np.uint64)
    lib.mi_debug_read_trace_ce.argtypes = [C.c_void_p, C.c_size_t]
    lib.mi_debug_read_trace_ce(buf.ctypes.data, buf.nbytes)
    t = buf.reshape(1024, 8)
    for i, n in enumerate(PHASES):
        v = t[:, i].astype(np.int64)
        print(f"      {n:32s} {np.median(v):9.0f} {np.percentile(v, 10):9.0f} {np.percentile(v, 90):9.0f}")
    w = t[:, 7]
    w0 = ((w >> np.uint64(32)) & np.uint64(0xffffffff)).astype(np.int64); w1 = (w & np.uint64(0xffffffff)).astype(np.int64)
    ok = w1 > 0
    base = w0[ok].min()
    print("      wall: starts", np.percentile(w0[ok] - base, [0, 50, 90, 100]) / 100.0, "us, ends", np.percentile(w1[ok] - base, [0, 50, 90, 100]) / 100.0,
          "us; life med %.1f us" % (np.median(w1[ok] - w0[ok]) / 100.0), "-> clock %.2f GHz" % (np.median(t[ok][:, :4].astype(np.int64).sum(1) / np.maximum((w1[ok] - w0[ok]) / 100.0, 1e-3)) / 1e3))


if mfma and not half and H % 2 == 0 and W % 4 == 0:
    wd, bd = torch.randn(8, 8, 4, 4, generator=g) * 0.1, torch.randn(8, generator=g)
    # the pair's second launch: the k4 s2 conv on CrossEmbed's output, on the kernel the engine picks (full-width stripes, else 8 x 32 tiles)
    cp = L.MiConvParams()
    cp.B, cp.H, cp.W = B, H // 2, W // 2
    cp.in0 = L.MiAct(out.data_ptr(), 8, ost.data_ptr(), nt, 1.0, 0)
    cp.Cout, cp.ksize, cp.stride = 8, 4, 2
    wf, cp.w_rp_exp = P.pack_conv_weight_rp(wd)
    wf, bdd = wf.to(dev), bd.to(dev)
    cp.w_rp, cp.bias = wf.data_ptr(), bdd.data_ptr()
    rows = lib.mi_conv_stripe_rows(C.byref(cp))
    ccfg, cnt = (12, (H // 2) // rows) if rows else (7, -(-(H // 2) // 8) * -(-(W // 2) // 32))
    dout = torch.empty(B, 8, H // 2, W // 2, device=dev)
    dst = torch.zeros(B, 8, cnt, 2, dtype=torch.float64, device=dev)
    cp.out, cp.out_stats, cp.tile_cfg = dout.data_ptr(), dst.data_ptr(), ccfg | 0x100
    us_d = timed(lib.mi_conv_fwd, cp, "conv")
    print(f"conv k4s2 8->8 @{H // 2}x{W // 2} B{B} tile_cfg {ccfg}: {us_d:.1f} us; the pair: {us + us_d:.1f} us")
    w9, b9 = P.compose_init_down(ws, [b_.cpu() for b_ in bs], wd, bd, 0, 3)
    tab9, exp9, b32 = P.pack_init_down_mfma(w9, b9)
    tab9, b32 = tab9.to(dev), b32.to(dev)
    add2 = torch.randn(B, 8, H // 2, W // 2, generator=g).to(dev)
    for icfg in (0, 1):
        q = L.MiInitDownParams()
        q.B, q.H, q.W, q.in0, q.C0, q.n_kernels = B, H, W, x.data_ptr(), 3, 3
        for i, (k, co) in enumerate(zip((3, 7, 15), (4, 2, 2))):
            q.ksize[i], q.cout[i] = k, co
        q.Cout, q.w_tab, q.w_exp, q.bias9 = 8, tab9.data_ptr(), exp9, b32.data_ptr()
        fnt = lib.mi_init_down_tiles(icfg, H, W)
        fout = torch.empty(B, 8, H // 2, W // 2, device=dev)
        fst = torch.zeros(B, 8, fnt, 2, dtype=torch.float64, device=dev)
        q.out, q.out_stats, q.tile_cfg, q.addend = fout.data_ptr(), fst.data_ptr(), icfg, add2.data_ptr()
        us_f = timed(lib.mi_init_down_fwd, q, "init_down")
        print(f"fused init_down B{B} {H}x{W} -> {H // 2}x{W // 2} tile_cfg {icfg}: {us_f:.1f} us ({(us + us_d) / us_f:.2f}x the pair)")
        trace()
    for _ in range(3):                      # (leave the CrossEmbed launch as the last one for the trace below)
        L.check(lib.mi_crossembed_fwd(C.byref(p), st), "crossembed")
    torch.cuda.synchronize()
trace()
