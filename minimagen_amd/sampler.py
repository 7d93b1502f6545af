"""The cascade's reverse-diffusion loop on the device (minimagen/Imagen.py:261-420): what a stage keeps between calls (StageState, on its
workspace), the launcher of one step's tail kernels, and the captured HIP graphs that replay [U-Net -> tail -> step advance].
What a stage of a call asks for arrives as ONE ``sample_call.StageCall`` (its defaults: the reference's loop); ``Imagen._stage_state`` /
``_stage_begin`` / ``_p_sample_loop`` delegate here and pass the knobs of Imagen.py (read there at call time)."""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _lib as L
from .helpers import cubic_taps, quantile_rank
from .sample_call import Noise, StageCall, graph_key, guidance_plan, guidance_scale_table, init_start_step  # noqa: F401  (host helpers, reachable as before)


def _drain(dev):
    if L.backend() == "hip-gfx950" and torch.cuda.is_available():
        torch.cuda.synchronize(dev)


def destroy_graph(entry, dev):
    """Drain the device, then destroy the captured graph exec of ``entry`` (a dict with a raw handle under "graph"): the one place graph
    execs go, for every cache in the package.  sample() never host-syncs its stage streams, so replays of the exec (and the buffers it
    addresses, dropped together with it) may still be queued -- all rare: new weights / .to(), a 9th graph, plan or solver setting."""
    if entry.get("graph") is not None:
        _drain(dev)
        L.lib().mi_graph_destroy(entry["graph"])
        entry["graph"] = None


def cubic_resize(ws, img, image_size: int, stream):
    """``img`` [B, C, H, W] at the workspace's image size through mi_resize_fwd (helpers.cubic_taps: antialiased when shrinking); ``img`` itself
    when the size already matches.  Tap tables: built and uploaded once per (workspace, source size) -- an upload from pageable host memory
    per call would block the host behind the previous call still running on this stage's stream."""
    B, Cc, Hin, Win = img.shape
    if Hin == image_size:
        return img
    cache = ws.resize_tabs
    if (Hin, Win) not in cache:
        _, idx_h, w_h = cubic_taps(Hin, image_size)
        _, idx_w, w_w = cubic_taps(Win, image_size)
        cache[(Hin, Win)] = ([t.to(ws.dev) for t in (idx_h, w_h, idx_w, w_w)], idx_h.shape[1], idx_w.shape[1])
    tabs, kh, kw = cache[(Hin, Win)]
    up = torch.empty(B, Cc, image_size, image_size, dtype=torch.float32, device=ws.dev)
    rp = L.MiResizeParams(B * Cc, Hin, Win, image_size, image_size, kh, kw, L.ptr(img), L.ptr(up),
                          L.ptr(tabs[0]), L.ptr(tabs[1]), L.ptr(tabs[2]), L.ptr(tabs[3]))
    L.check(L.lib().mi_resize_fwd(C.byref(rp), stream), "mi_resize_fwd")
    ws.resize_keepalive = tabs
    return up


class StageState:
    """One stage's loop state, kept on its workspace (so it dies with the buffers it points into) per schedule -- or per (schedule, S, sampler, eta) for a call with
    ``solver`` = (S, sampler, eta).  Every field is a slot; ``ext`` and ``group_sync`` stay UNSET until they exist (``hasattr`` is how callers ask for a solver
    extension / a grouped tail); ``t_map`` / ``group_err_host``, None until then, answer the same here. ``hw`` (pixels per channel plane) makes it the state of an
    INPAINTING call -- an entry of its own: the coefficient table with columns 6 and 7, and the known-image / mask buffers every call copies into (so one captured
    graph serves every later call's images and masks); ``ip`` (None otherwise) is the kernels' block over them, rebuilt by every stage_begin.  ``objective`` (what
    the stage's U-Net predicts: 'noise', 'x_start' or 'v') only chooses columns 0 and 1 of the coefficient table: no kernel, struct or launch knows about it.
    ``rescale_partials`` (None until a call with guidance_rescale > 0 runs on this state): the [B][chunks][4] fp64 sums of mi_cfg_rescale_*. ``scale_tab`` (None
    until a 'table' run of a guidance schedule runs on this state): fp32 [S][B], row k the scales of step index k, which every such call copies
    into -- the captured graphs address it, so they serve every later call's values."""
    __slots__ = ("coef", "tau", "t_map", "x0_prev", "ext", "t_state", "x0", "hist", "s_q", "v_q", "seed_dev", "graphs",
                 "group_sync", "group_err_host", "group_failed", "group_heal", "known", "mask", "ip", "known_noise", "rescale_partials", "scale_tab", "scale_tab_host")

    def __init__(self, sched, B: int, n: int, dev, solver=None, hw: int = None, objective: str = 'noise', start: int = 0):
        self.tau = self.t_map = self.x0_prev = None     # the reference's loop has no step -> timestep map and no history
        self.known = self.mask = self.ip = self.known_noise = self.rescale_partials = self.scale_tab = self.scale_tab_host = None
        known = {} if hw is None else dict(known=True)
        if objective != 'noise':
            known['objective'] = objective
        if hw is not None:
            self.known = torch.zeros(B, n, dtype=torch.float32, device=dev)
            self.mask = torch.zeros(B, hw, dtype=torch.uint8, device=dev)
        if solver is None:
            self.coef = sched.sampler_coef_table(**known).to(dev).contiguous()
        else:
            if start and solver[1] == 'dpmpp_2m':             # a loop that skips its first steps: the first one executed is first order
                known['start'] = start
            self.tau, coef = sched.sampler_tables(solver[0], solver[1], solver[2] if solver[1] == 'ddim' else None, **known)
            self.coef = coef.to(dev).contiguous()
            self.t_map = self.tau.to(torch.int32).to(dev).contiguous()
            if solver[1] == 'dpmpp_2m':
                self.x0_prev = torch.zeros(B, n, dtype=torch.float32, device=dev)
            self.ext = L.MiSamplerExtParams(L.ptr(self.t_map), L.ptr(self.x0_prev))
        self.t_state = torch.zeros(1, dtype=torch.int32, device=dev)        # the device-resident step
        self.x0 = torch.empty(B, n, dtype=torch.float32, device=dev)
        self.hist = torch.zeros(3 * B * 2 * 2048, dtype=torch.int32, device=dev)
        self.s_q = torch.zeros(B, dtype=torch.float32, device=dev)
        self.v_q = torch.zeros(B, 2, dtype=torch.float32, device=dev)
        self.seed_dev = None            # the Philox seed in device memory (on-device noise): replays of later calls need no re-capture
        self.graphs = {}                # graph key -> dict(step, graph, keep, per)
        self.group_err_host = None      # the pinned copy of the grouped tail's error word, allocated with its sync buffer (group_sync)
        self.group_failed = self.group_heal = False         # a grouped launch gave up: separate kernels from then on / re-zero the buffer

    def close(self, dev):
        """Drain the device and destroy the captured graph execs (raw handles, not tensors)."""
        _drain(dev)
        for entry in self.graphs.values():
            destroy_graph(entry, dev)
        self.graphs.clear()


def stage_state(ws, sched, shape, call: StageCall, eng=None, max_states: int = 8) -> StageState:
    """The workspace's state for this call's stage: keyed by ``call.state_key`` -- T for the default call; every other key is a tuple, and those
    states (solver settings, inpainting, objectives) are bounded together.  ``shape`` = (B, C, H, W)."""
    store = ws.sampler_state
    key = call.state_key(sched.num_timesteps)
    bounded = isinstance(key, tuple)
    st = store.get(key)
    if st is not None and bounded:
        store[key] = store.pop(key)                      # most recently used last
    if st is None and bounded:
        # bounded: a caller sweeping S or eta must not grow device memory (a status word still to be polled keeps its state object alive)
        solver_keys = [k for k in store if isinstance(k, tuple)]
        while len(solver_keys) >= max_states:
            old = store.pop(solver_keys.pop(0))
            old.close(ws.dev)
            if eng is not None:
                eng.drop_step_tables(ws, old.t_state)
    if st is None:
        st = store[key] = StageState(sched, shape[0], shape[1] * shape[2] * shape[3], ws.dev, call.solver, None if call.inpaint is None else shape[2] * shape[3],
                                     call.objective, call.start)
    return st


def known_begin(st: StageState, ws, shape, inpaint, *, sched, known_noise, seed: int, sample0: int, stage: int, stream, start: int = 0, steps: int = None):
    """The known region of an inpainting call at this stage: the caller's images resized to the stage's size (cubic taps), clamped to [0, 1] and normalised INTO
    st.known, the masks resized (nearest) into st.mask, and blend 0 on the x_T just drawn: the known pixels at the noise level of x_T.  ``inpaint`` = (images float32
    [B, C, H, W], masks uint8 [B, Hm, Wm], normalize), on the device. ``start`` = a0 > 0 (the loop of ``steps`` steps begins at step a0 on an init-noised x): blend 0
    at THAT level, with the known-region draw a0 -- the one the tail of step a0 - 1 would have used -- through a copy of the block whose stream and buffer are moved
    on by a0."""
    lib = L.lib()
    images, masks, normalize = inpaint
    B, Cc, H, W = shape
    n = Cc * H * W
    at_size = cubic_resize(ws, images, H, stream)
    L.check(lib.mi_inpaint_prepare_fwd(L.ptr(at_size), L.ptr(st.known), B, n, 1 if normalize else 0, L.ptr(masks), masks.shape[1], masks.shape[2],
                                       L.ptr(st.mask), H, stream), "mi_inpaint_prepare_fwd")
    st.known_noise = known_noise          # (st.ip holds its address: an injected buffer lives until the next call's)
    st.ip = L.MiInpaintParams(L.ptr(st.known), L.ptr(st.mask), H * W, (stage << 20) | (3 << 18), L.ptr(known_noise))
    ip0 = st.ip
    if start:
        a, b = sched.init_start_coefs(steps, start)
        ip0 = L.MiInpaintParams.from_buffer_copy(st.ip)
        ip0.known_stream += start
        if known_noise is not None:
            ip0.known_noise = L.ptr(known_noise) + start * B * n * 4
    else:
        a, b = sched.known_start_coefs()
    L.check(lib.mi_inpaint_blend0_fwd(L.ptr(ws.x), B, n, C.byref(ip0), a, b, int(seed) & 0x7FFFFFFFFFFFFFFF, sample0, stream), "mi_inpaint_blend0_fwd")


def stage_begin(unet, shape, ws, call: StageCall, *, noise_scheduler, noise: Noise = Noise(), max_states: int = 8):
    """Everything of a stage's loop that does not depend on the PREVIOUS stage's image: x_T (Imagen.py:400), the device-resident timestep, the per-step conditioning
    tables of all T steps -- and, for an inpainting call (``call.inpaint``: see known_begin), the stage's known image and mask and blend 0. ``noise``: where the
    draws come from (sample_call.Noise).  sample() issues it for every stage before the first stage's loop, so that a later stage's stream has it done while it waits
    for its low-resolution input (on-device noise only: injected noise is drawn in the reference's order, then the T known-region draws). ``call.init`` = (images
    float32 [B, C, H, W] on the device, normalize) with ``call.start`` = a0: the loop begins at step a0 on x = a y' + b eps -- y' the images at
    the stage's size in the sampler's range, (a, b) the level of the first executed step (init_start_coefs), eps the stage's OWN x_T draw (same Philox stream and
    keying, or the same noise_fn call), made by ONE launch (mi_init_noise_fwd) in place of the x_T fill; every other draw keeps its index, the device step index
    becomes T - 1 - a0."""
    lib, stream, eng = L.lib(), L.current_stream(), unet.engine()
    B, n = shape[0], shape[1] * shape[2] * shape[3]
    (noise_fn, seed, sample0), stage, solver, inpaint, start, init = noise, call.stage, call.solver, call.inpaint, call.start, call.init
    T = call.steps                                                           # steps of the loop (one draw each, for every solver)
    assert 0 <= start < T and (init is not None or not start), (start, T)
    st = stage_state(ws, noise_scheduler, shape, call, eng, max_states)
    noise_dev = known_noise = None
    x_t_stream = (stage << 20) | (1 << 19) | 1

    def init_noise(eps):                                                     # x = a y' + b eps (eps None: the x_T draw, generated in the launch)
        at_size = cubic_resize(ws, init[0], shape[2], stream)
        a, b = noise_scheduler.init_start_coefs(None if solver is None else T, start)
        L.check(lib.mi_init_noise_fwd(L.ptr(at_size), L.ptr(ws.x), B, n, 1 if init[1] else 0, a, b, seed, sample0, x_t_stream, L.ptr(eps), stream),
                "mi_init_noise_fwd")

    if noise_fn is not None:
        if init is None:
            ws.x.copy_(noise_fn(shape))                                      # Imagen.py:400
        else:
            init_noise(noise_fn(shape).to(ws.dev, torch.float32).contiguous())
        noise_dev = torch.stack([noise_fn(shape) for _ in range(T)]).to(ws.dev).contiguous()   # Imagen.py:361, in step order
        if inpaint is not None:
            known_noise = torch.stack([noise_fn(shape) for _ in range(T)]).to(ws.dev).contiguous()   # blends 0 .. T-1
    elif init is None:
        L.check(lib.mi_randn_fill(L.ptr(ws.x), B, n, seed, sample0, x_t_stream, stream), "mi_randn_fill")
    else:
        init_noise(None)
    if inpaint is not None:
        known_begin(st, ws, shape, inpaint, sched=noise_scheduler, known_noise=known_noise, seed=seed, sample0=sample0, stage=stage, stream=stream,
                    start=start, steps=None if solver is None else T)
    if st.t_map is None:
        L.check(lib.mi_step_set(L.ptr(st.t_state), L.ptr(ws.times), B, T - 1 - start, stream), "mi_step_set")
    else:
        # the device-resident state is the STEP index; the U-Net's conditioning sees the trained timestep t_map[step]
        L.check(lib.mi_step_set_mapped(L.ptr(st.t_state), L.ptr(ws.times), B, T - 1 - start, C.byref(st.ext), stream), "mi_step_set_mapped")
    if st.x0_prev is not None:
        st.x0_prev.zero_()                                       # the first step's history coefficient is 0: 0 * stale must not be NaN
    eng.prepare_step_tables(ws, T, st.t_state, stream, t_map=st.tau)         # (timestep, text)-only conditioning of all T steps, once
    return st, noise_dev


def stage_attach(unet, shape, ws, call: StageCall, *, noise_scheduler, first: StageState, max_states: int = 8) -> StageState:
    """The state of a FURTHER workspace a stage visits in this call (a guidance plan of several runs), behind stage_begin on the first one: its step
    tables, and for an inpainting call its known image and mask, copied from ``first`` (resized once) over the same known-region noise.  No draw: x, the history and
    the step index arrive with the hand-over (stage_handover)."""
    eng = unet.engine()
    st = stage_state(ws, noise_scheduler, shape, call, eng, max_states)
    if call.inpaint is not None:
        st.known.copy_(first.known)
        st.mask.copy_(first.mask)
        st.known_noise = first.known_noise
        st.ip = L.MiInpaintParams(L.ptr(st.known), L.ptr(st.mask), shape[2] * shape[3], (call.stage << 20) | (3 << 18), L.ptr(st.known_noise))
    eng.prepare_step_tables(ws, call.steps, st.t_state, L.current_stream(), t_map=st.tau)
    return st


def stage_handover(src: StageState, ws_src, dst: StageState, ws_dst, B: int, step: int):
    """A run boundary on the stage's stream, outside the graphs: x (and the x0 history of dpmpp_2m) of the run that ended go to the next run's
    workspace, whose device-resident step index becomes ``step`` -- the index the host knows.  Plain device copies."""
    lib, stream = L.lib(), L.current_stream()
    ws_dst.x.copy_(ws_src.x)
    if dst.x0_prev is not None:
        dst.x0_prev.copy_(src.x0_prev)
    if dst.t_map is None:
        L.check(lib.mi_step_set(L.ptr(dst.t_state), L.ptr(ws_dst.times), B, step, stream), "mi_step_set")
    else:
        L.check(lib.mi_step_set_mapped(L.ptr(dst.t_state), L.ptr(ws_dst.times), B, step, C.byref(dst.ext), stream), "mi_step_set_mapped")


def tail_launcher(st: StageState, ws, kind: str, cp, qp, pp, stream, clip: int = None):
    """What follows the U-Net evaluation in a step, fixed once per graph entry -> (launch, advance): ``launch(k)`` enqueues the tail kernels of
    step *t_state - k (``kind``: "small" one workgroup per image | "group" cooperating workgroups | "separate" kernels | "direct" the one elementwise launch
    of a stage without the dynamic threshold, ``clip`` = 1 static clamp / 0 none: mi_sampler_step_direct_fwd, at every image size), ``advance(n)`` moves the
    device-resident step by n (mapped entries when the state has a step -> timestep map).  Always the *_ext_fwd tails: without st.ext / a history buffer they ARE the plain ones;
    the *_inpaint_fwd tails for the state of an inpainting call (chosen here, once: a step has no branch for it)."""
    lib, tails = L.lib(), {}
    ext, q_ = (C.byref(st.ext) if st.t_map is not None else None), C.byref(qp)
    state = (L.ptr(st.t_state), L.ptr(ws.times), cp.B)
    form, blocks = ("ext", (ext,)) if st.ip is None else ("inpaint", (ext, C.byref(st.ip)))
    small_fwd, group_fwd, posterior_fwd = (getattr(lib, f"mi_{name}_{form}_fwd") for name in ("sampler_step_small", "sampler_step_group", "posterior"))

    def params(k):
        if k not in tails:
            c_, p_ = L.MiCfgX0Params.from_buffer_copy(cp), L.MiPosteriorParams.from_buffer_copy(pp)
            c_.t_off = p_.t_off = k
            if kind != "separate":
                c_.x0 = c_.hist0 = 0                      # x0 stays in registers, the histograms in LDS (and per-image counters)
            tails[k] = (C.byref(c_), q_, C.byref(p_))                # (the references keep the blocks alive)
        return tails[k]

    def small(k=0):
        L.check(small_fwd(*params(k), *blocks, stream), f"mi_sampler_step_small_{form}_fwd")

    def group(k=0):
        L.check(group_fwd(*params(k), *blocks, L.ptr(st.group_sync), stream), f"mi_sampler_step_group_{form}_fwd")

    def separate(k=0):
        c_, _, p_ = params(k)
        L.check(lib.mi_cfg_x0_fwd(c_, stream), "mi_cfg_x0_fwd")
        L.check(lib.mi_quantile_fwd(q_, stream), "mi_quantile_fwd")
        L.check(posterior_fwd(p_, *blocks, stream), f"mi_posterior_{form}_fwd")

    def direct(k=0):
        c_, _, p_ = params(k)
        L.check(lib.mi_sampler_step_direct_fwd(c_, p_, ext, None if st.ip is None else C.byref(st.ip), clip, stream), "mi_sampler_step_direct_fwd")

    if st.t_map is None:
        advance = lambda n=1: L.check(lib.mi_step_advance_by(*state, n, stream), "mi_step_advance_by")
    else:
        advance = lambda n=1: L.check(lib.mi_step_advance_by_mapped(*state, n, ext, stream), "mi_step_advance_by_mapped")
    return dict(small=small, group=group, separate=separate, direct=direct)[kind], advance


def run_plan(im, unet, shape, workspaces, call: StageCall, begun, *, max_states: int = 8, **loop):
    """A stage whose guidance plan has several runs, or reads its scales from a table: every run on the workspace of its kind
    (``workspaces``: kind -> workspace), x / the history / the step index handed over at the run boundaries, one noise stream (``begun``: the stage_begin of
    the first run's workspace, issued here for injected noise) -> the image.  ``loop``: noise_scheduler, noise and use_graph, as p_sample_loop takes them."""
    runs, first = call.runs, workspaces[call.runs[0][0]]
    if begun is None:
        begun = im._stage_begin(unet, shape, first, call, noise_scheduler=loop["noise_scheduler"], noise=loop["noise"])
    st0, noise_dev = begun
    states = {kind: st0 if ws is first else stage_attach(unet, shape, ws, call, noise_scheduler=loop["noise_scheduler"], first=st0, max_states=max_states)
              for kind, ws in workspaces.items()}
    img = prev = None
    for run in runs:
        kind, a = run[:2]
        if prev is not None:
            stage_handover(states[prev], workspaces[prev], states[kind], workspaces[kind], shape[0], call.steps - 1 - a)
        img = im._p_sample_loop(unet, shape, workspaces[kind], call, run, begun=(states[kind], noise_dev), finalize=run is runs[-1], **loop)
        prev = kind
    return img


def p_sample_loop(im, unet, shape, ws, call: StageCall, run=None, *, noise_scheduler, noise: Noise = Noise(), use_graph: bool = True, begun=None,
                  finalize: bool = True, group_max: int = 8, max_states: int = 8):
    """Imagen.py:373-420 + :329-370 + :261-326: T replays of [U-Net (both guidance halves) -> CFG combine + x0 -> dynamic-threshold quantile (``call.threshold`` 'dynamic'; 'static' / 'none': no select, the one-launch direct tail) -> posterior draw -> t -=
    1].  ``call.solver`` = (S, sampler, eta): S steps over a subsequence of the trained timesteps; the loop, the noise index and the Philox stream count STEPS: the
    reference's loop with T = S but for the state's step -> timestep map and history buffer (``st.ext``). ``call.objective``: what the U-Net predicts; it selects the
    stage state (its coefficient table) and nothing else. ONE RUN of the stage's guidance plan, ``run`` = (kind, a, b, scale), default the
    stage's only one: the steps a .. b - 1 of the T (counted from the first executed; the state's step index is T - 1 - a on entry: stage_begin or stage_handover put
    it there) at cond_scale = ``scale`` -- or, kind 'table' (on a workspace built with fold=False), at the scales of ``call.scales`` (host float [T] or [T, B] in
    execution order), read per step and row from the state's ``scale_tab`` by mi_cfg_sched_combine_fwd or the sched forms of the rescale launches; ``finalize=False``
    returns None instead of the image. ``call.rescale`` = phi > 0 on a guided run (on a workspace built with fold=False): two launches between the
    U-Net and the tail leave the rescaled guided prediction in rows [0, B) of ws.pred, and the tail runs as it does behind a folded U-Net.  ``call.init``
    (stage_begin) only matters when the stage has not begun yet (``begun`` None: injected noise): the run itself is a run (a0, T) like any other."""
    lib, stream, eng = L.lib(), L.current_stream(), unet.engine()
    (B, Cc, H, W), T, stage, sample0 = shape, call.steps, call.stage, noise.sample0
    n = Cc * H * W
    kind_of_run, a_step, b_step, cond_scale = call.runs[0] if run is None else run
    sched = kind_of_run == 'table'
    cond_scale, scale_tab = (1., call.scales) if sched else (cond_scale, None)
    two = ws.B2 != ws.B
    eng.set_guidance(ws, cond_scale)
    rescale = float(call.rescale) if kind_of_run != 'plain' else 0.
    assert not (rescale or sched) or (two and ws.cfg_fold is None), "guidance rescale / a table of guidance scales reads both halves of the prediction"
    combine = two and ws.cfg_fold is None and not rescale and not sched   # guidance folded into the U-Net's tail / rescaled / combined in place: ws.pred holds B guided rows
    if begun is None:
        begun = stage_begin(unet, shape, ws, call, noise_scheduler=noise_scheduler, noise=noise, max_states=max_states)
    st, noise_dev = begun
    assert 0 <= a_step < b_step <= T, run
    m_steps = b_step - a_step
    if sched:                                # every call's values go into the buffer the captured launches address (row k: step index k)
        if st.scale_tab is None:
            st.scale_tab = torch.ones(T, B, dtype=torch.float32, device=ws.dev)
        tab = torch.as_tensor(scale_tab, dtype=torch.float32).reshape(T, -1).expand(T, B).flip(0).contiguous()
        # (a copy from pageable host memory blocks the host behind this stream: skipped when the values are the ones already there)
        if st.scale_tab_host is None or not torch.equal(st.scale_tab_host, tab):
            st.scale_tab.copy_(tab)
            st.scale_tab_host = tab
    rank = k_lo, k_hi, w = quantile_rank(n, im.dynamic_thresholding_percentile if call.percentile is None else call.percentile)
    # the whole tail in one launch: of one workgroup per image (n <= MI_SAMPLER_SMALL_N), or of <= group_max (0: never) cooperating workgroups -- but
    # for a stage state whose grouped launch ever failed (fail-stop: NaN images + the sticky error word, see Imagen._poll_status).  A stage without the
    # dynamic threshold has nothing to select: "direct", ONE elementwise launch at every size, whatever the knobs say
    fused = os.environ.get("MINIMAGEN_SAMPLER_FUSED", "1") != "0"
    grouped = fused and 0 < lib.mi_sampler_group_size(n) <= group_max and not st.group_failed
    clip = {'dynamic': None, 'static': 1, 'none': 0}[call.threshold]
    kind = "direct" if clip is not None else "small" if (fused and n <= 16384) else "group" if grouped else "separate"
    group = kind == "group"
    if st.group_heal:
        st.group_sync.zero_()               # stream-ordered behind every launch queued on this lane: ticket, counters, histograms, error word
        st.group_heal = False
    seed = int(noise.seed) & 0x7FFFFFFFFFFFFFFF
    if noise_dev is None:
        if st.seed_dev is None:
            st.seed_dev = torch.zeros(1, dtype=torch.int64, device=ws.dev)
        st.seed_dev.fill_(seed)
    # the captured graph of `per` steps is cached per sample_call.graph_key (the seed is in device memory);
    # `per` steps per captured graph (one replay boundary, ~9 us of idle GPU, per graph): step k addresses *t_state - k, one advance per graph
    cap = int(os.environ.get("MINIMAGEN_STEPS_PER_GRAPH", "5"))
    if m_steps == T:
        per = next(k for k in (5, 4, 3, 2, 1) if k <= cap and T % k == 0)
        lengths = [per] * (T // per)
    else:                                    # a run of a plan: m // per graphs of per steps and one of m % per; such a graph's key carries its length
        per = max(1, min(cap, 5, m_steps))
        lengths = [per] * (m_steps // per) + ([m_steps % per] if m_steps % per else [])
    keys = {length: graph_key(call, cond_scale, two, rank, sample0, noise_dev is None, group, st.ip is not None, rescale, sched, None if m_steps == T else length)
            for length in (lengths if use_graph else lengths[:1])}
    if use_graph and noise_dev is None:
        # bounded: one exec per (guidance, threshold, shard offset) combination and length; the oldest go, never one this run replays
        missing = sum(1 for k in keys.values() if k not in st.graphs)
        victims = [k for k in st.graphs if k not in keys.values()]
        while missing and victims and len(st.graphs) + missing > 8:
            destroy_graph(st.graphs.pop(victims.pop(0)), ws.dev)
    entries = {}
    for length, key in keys.items():
        entries[length] = _loop_entry(im, unet, st, ws, key, length, B=B, n=n, T=T, two=two, combine=combine, cond_scale=cond_scale, rescale=rescale, sched=sched,
                                      kind=kind, clip=clip, group=group, k_lo=k_lo, k_hi=k_hi, w=w, noise_dev=noise_dev, seed=seed, sample0=sample0, stage=stage, use_graph=use_graph)
    if use_graph:
        try:
            for length in lengths:
                L.check(lib.mi_graph_launch(entries[length]["graph"], stream), "mi_graph_launch")
        finally:
            if noise_dev is not None:          # one-off graphs (injected noise buffer): the execs must outlive their replays
                for entry in entries.values():
                    destroy_graph(entry, ws.dev)
    else:
        for _ in range(m_steps):
            entries[lengths[0]]["step"]()
    if group:
        # the sticky error word goes to pinned host memory behind the stage's last launch; Imagen._poll_status reads it once this call's event has fired
        st.group_err_host.copy_(st.group_sync[8:12].view(torch.int32), non_blocking=True)
        im._status_stages.append((st, stage, (B, H, W)))
    if not finalize:
        return None
    img = torch.empty(shape, dtype=torch.float32, device=ws.dev)
    L.check(lib.mi_finalize_images(L.ptr(ws.x), L.ptr(img), B * n, 1 if im.auto_normalize_img else 0, stream), "mi_finalize_images")
    return img


def _loop_entry(im, unet, st, ws, gkey, per, *, B, n, T, two, combine, cond_scale, rescale, sched, kind, clip, group, k_lo, k_hi, w, noise_dev, seed,
                sample0, stage, use_graph):
    """The cached (or, for injected noise and eager runs, one-off) entry of ``per`` steps of p_sample_loop: dict(step, graph, per)."""
    lib, stream, eng = L.lib(), L.current_stream(), unet.engine()
    entry = st.graphs.get(gkey) if (use_graph and noise_dev is None) else None
    if entry is None:
        # the radix select's first pass rides on the producer of x0; st.hist is zero on allocation and every mi_quantile_fwd leaves it zeroed again
        cp = L.MiCfgX0Params(B, n, L.ptr(ws.pred), 1 if combine else 0, float(cond_scale), L.ptr(ws.x), L.ptr(st.coef), L.ptr(st.t_state), 0, L.ptr(st.x0), L.ptr(st.hist))
        qp = L.MiQuantileParams(B, n, L.ptr(st.x0), k_lo, k_hi, w, L.ptr(st.hist), L.ptr(st.s_q), L.ptr(st.v_q), 1, 1)
        pp = L.MiPosteriorParams(B, n, T, L.ptr(st.x0), L.ptr(st.s_q), L.ptr(ws.x), L.ptr(st.coef), L.ptr(st.t_state),
                                 L.ptr(noise_dev), seed, sample0, stage << 20, L.ptr(st.seed_dev) if noise_dev is None else 0)
        if group and st.group_err_host is None:
            st.group_sync = torch.zeros(lib.mi_sampler_group_sync_bytes(B, n), dtype=torch.uint8, device=ws.dev)   # this workspace's launches only
            st.group_err_host = torch.zeros(1, dtype=torch.int32).pin_memory() if L.backend() == "hip-gfx950" else torch.zeros(1, dtype=torch.int32)
        launch, advance = tail_launcher(st, ws, kind, cp, qp, pp, stream, clip)
        rp, sps = None, {}
        if rescale and st.rescale_partials is None:
            st.rescale_partials = torch.zeros(B, lib.mi_cfg_rescale_chunks(n), 4, dtype=torch.float64, device=ws.dev)
        if rescale and not sched:                # phi and the scale are baked into the launches (gkey)
            rp = C.byref(L.MiCfgRescaleParams(B, n, L.ptr(ws.pred), float(cond_scale), rescale, L.ptr(st.rescale_partials)))

        def sched_params(k):                     # phi is baked in, the scales are read from st.scale_tab at step *t_state - k
            if k not in sps:
                sps[k] = L.MiCfgSchedParams(B, n, L.ptr(ws.pred), L.ptr(st.scale_tab), L.ptr(st.t_state), k, rescale, L.ptr(st.rescale_partials) if rescale else 0)
            return C.byref(sps[k])

        def one_step(k=0, by=1):                 # step *t_state - k, then the device-resident step moves by `by`
            eng.run_step(ws, stream, t_off=k)
            if rp is not None:
                L.check(lib.mi_cfg_rescale_stats_fwd(rp, stream), "mi_cfg_rescale_stats_fwd")
                L.check(lib.mi_cfg_rescale_apply_fwd(rp, stream), "mi_cfg_rescale_apply_fwd")
            elif sched and rescale:
                L.check(lib.mi_cfg_sched_rescale_stats_fwd(sched_params(k), stream), "mi_cfg_sched_rescale_stats_fwd")
                L.check(lib.mi_cfg_sched_rescale_apply_fwd(sched_params(k), stream), "mi_cfg_sched_rescale_apply_fwd")
            elif sched:
                L.check(lib.mi_cfg_sched_combine_fwd(sched_params(k), stream), "mi_cfg_sched_combine_fwd")
            launch(k)
            if by:
                advance(by)
        entry = dict(step=one_step, graph=None, per=per)
        if use_graph:
            offsets = eng.step_offsets_supported(ws)
            L.check(lib.mi_graph_begin(stream), "mi_graph_begin")
            try:
                for k in range(per):
                    one_step(k, per if k == per - 1 else 0) if offsets else one_step()
            finally:
                g = C.c_void_p()
                rc = lib.mi_graph_end(stream, C.byref(g))
            L.check(rc, "mi_graph_end")
            entry["graph"] = g
            if noise_dev is None:
                st.graphs[gkey] = entry
    return entry
