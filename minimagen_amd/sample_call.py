"""What a call of ``Imagen.sample()`` IS, worked out on the host before anything is launched: the validation of its keywords (``parse_*`` =
``Imagen._parse_*``), the host arithmetic of init images and guidance schedules, and the two records the rest of the package reads --
``SampleCall`` (what every stage shares) and one frozen ``StageCall`` per stage that runs.  A feature that is off is a field at its default: the
default ``StageCall`` IS the reference's loop, with the state key and graph key (each built in ONE place, below) it always had.  Never imports ``_lib``."""
from __future__ import annotations

import dataclasses
import os
from typing import Callable, NamedTuple, Optional

import torch

from .diffusion_model import GaussianDiffusion


def is_number(v) -> bool:                        # a real number: an int or a float, not a bool
    return not isinstance(v, bool) and isinstance(v, (int, float))


def reject(when, message: str):
    if when:
        raise ValueError(message)


def per_stage(v, n: int, name: str, single=None, noun: str = "value", unit: str = "stage", counted: bool = True) -> list:
    """One value for every stage (``single(v)``, default: anything but a list / tuple) or a list / tuple with one per stage -> a list of ``n``."""
    if single(v) if single is not None else not isinstance(v, (list, tuple)):
        return [v] * n
    reject(not isinstance(v, (list, tuple)) or len(v) != n, f"{name} needs one {noun} per {unit} ({n})" + (f", got {len(v)}" if counted else ""))
    return list(v)


def pixel_images(t, name: str, batch: int, channels: int) -> torch.Tensor:
    """The caller's images (``inpaint_images``, ``start_image``, ``init_images``): float [batch, channels, H, H] -> float32, where they are."""
    reject(not torch.is_tensor(t) or t.dim() != 4 or not t.is_floating_point(), f"{name} must be a float tensor [B, {channels}, H, W]")
    reject(t.shape[0] != batch, f"{name}: batch {t.shape[0]} does not match the text batch {batch}")
    reject(t.shape[1] != channels, f"{name}: {t.shape[1]} channels, the model has {channels}")
    reject(t.shape[2] != t.shape[3] or t.shape[2] < 1, f"{name} must be square, got {tuple(t.shape[2:])}")
    return t.detach().to(torch.float32)


def init_start_step(steps: int, strength: float) -> int:
    """a0, the number of steps a loop of S = ``steps`` steps skips when it starts from an init image at ``strength`` in (0, 1]: it executes its
    last m = min(S, max(1, floor(strength S + 0.5))) steps, a0 = S - m (strength 1: the whole loop).  Host only; raises ValueError."""
    S = int(steps)
    reject(not is_number(strength) or not 0. < float(strength) <= 1., f"init_strength must be a number in (0, 1], got {strength!r}")
    reject(S < 1, f"steps must be positive, got {steps!r}")
    return S - min(S, max(1, int(float(strength) * S + 0.5)))


def guidance_scale_table(tau, T: int, B: int, cond_scale: float = 1., interval=None, schedule=None) -> torch.Tensor:
    """A stage's guidance scales in EXECUTION order (entry 0: the first step executed, the noisiest one), float64 [S] or [S, B] (per row; the caller's values as they
    are: a run at ONE scale is the call at that cond_scale, a table run rounds them to fp32). ``tau`` int64 [S]: the trained timestep of step index k
    (GaussianDiffusion.sampling_timestep_map; arange(T) for the reference's loop) -- entry i is the step at tau[S - 1 - i].  ``schedule``: None (``cond_scale`` on
    every step), a callable f(u) -> float with u = tau_k / (T - 1), or a tensor / sequence [S] or [S, B] already in execution order.  ``interval`` = (lo, hi): a step
    outside lo (T - 1) <= tau_k <= hi (T - 1) (float64 against the integer tau_k) gets scale 1.  Host only; raises ValueError on bad values."""
    taus = [int(v) for v in reversed(tau.tolist())]
    S = len(taus)
    if schedule is None:
        w = torch.full((S,), float(cond_scale), dtype=torch.float64)
    elif callable(schedule):
        vals = []
        for t in taus:
            v = schedule(t / (T - 1))
            reject(not is_number(v), f"guidance_schedule: the callable must return a float, got {v!r}")
            vals.append(float(v))
        w = torch.tensor(vals, dtype=torch.float64)
    else:
        try:
            w = torch.as_tensor(schedule).detach().to('cpu')
        except Exception as e:
            raise ValueError(f"guidance_schedule: not a tensor or a sequence of numbers ({e})")
        if w.dtype == torch.bool or not (w.is_floating_point() or w.dtype in (torch.int32, torch.int64)):
            raise ValueError(f"guidance_schedule: a float tensor or sequence, got dtype {w.dtype}")
        w = w.to(torch.float64)
        if w.dim() not in (1, 2) or w.shape[0] != S or (w.dim() == 2 and w.shape[1] != B):
            raise ValueError(f"guidance_schedule: shape {tuple(w.shape)} is neither [{S}] (one scale per step executed) nor [{S}, {B}] (per row)")
    reject(not bool(torch.isfinite(w).all()), "guidance_schedule: the scales must be finite")
    if interval is not None:
        lo, hi = interval
        inside = torch.tensor([lo * (T - 1) <= t <= hi * (T - 1) for t in taus])
        w = torch.where(inside if w.dim() == 1 else inside[:, None], w, torch.ones_like(w))
    return w.contiguous()


def guidance_plan(w: torch.Tensor):
    """The runs of a stage whose guidance scales are ``w`` (float [S] or [S, B], execution order): a list of (kind, first step, one past the
    last step, scale), maximal runs of steps of one kind --
      'plain'   every row's scale is exactly 1: the B-row workspace, one U-Net row per image
      'scalar'  ONE row-uniform scale s != 1 (all the stage's guided steps share it): the existing guided path at cond_scale = s, folded where
                it folds today; ``scale`` = s
      'table'   anything else: the unfolded 2B-row workspace, the scale read per step and row from device memory (``scale`` = None)
    A single 'plain' or 'scalar' run over all S steps IS the existing call at cond_scale = 1 / s: same workspaces, states, graph keys, bits."""
    w2 = w.reshape(w.shape[0], -1).to(torch.float64)
    S = w2.shape[0]
    guided = [bool((w2[i] != 1.).any()) for i in range(S)]
    values = {float(v) for i in range(S) if guided[i] for v in w2[i].tolist()}
    one = len(values) == 1                       # (a guided step with a row at 1 beside another value has two values: a table)
    kind = lambda i: 'plain' if not guided[i] else ('scalar' if one else 'table')
    runs, i = [], 0
    while i < S:
        j = i
        while j < S and kind(j) == kind(i):
            j += 1
        runs.append((kind(i), i, j, 1. if kind(i) == 'plain' else (next(iter(values)) if one else None)))
        i = j
    return runs


class Noise(NamedTuple):
    """A call's draws: ``fn(shape)``, a host stream in the reference's draw order, or (None) Philox keyed by (seed, sample0 + row, stage, step, element)."""
    fn: Optional[Callable] = None
    seed: int = 0
    sample0: int = 0


@dataclasses.dataclass(frozen=True)
class StageCall:
    """One stage of one call.  Every default is the plain call: the reference's loop on all T timesteps, from pure noise, noise-predicting,
    no known pixels, ONE run of the guidance plan."""
    stage: int
    steps: int                                   # the loop's length: T, or S of ``solver``
    solver: Optional[tuple] = None               # (S, sampler, eta)
    start: int = 0                               # a0: the loop begins at step a0 on an init-noised x (``init``)
    objective: str = 'noise'                     # what the stage's U-Net predicts
    inpaint: Optional[tuple] = None              # (images float32 [B, C, H, W], masks uint8 [B, Hm, Wm], normalize)
    init: Optional[tuple] = None                 # (images float32 [B, C, H, W], normalize)
    runs: tuple = ()                             # the guidance plan, (kind, first step, one past the last, scale) (guidance_plan)
    scales: Optional[torch.Tensor] = None        # the stage's guidance scales, [S] or [S, B] in execution order, for its 'table' runs
    rescale: float = 0.                          # phi of guidance rescale, applied on the guided runs
    threshold: str = 'dynamic'                   # how x0 is bounded: 'dynamic' (the reference), 'static' (clamp to [-1, 1]) or 'none'
    percentile: Optional[float] = None           # the dynamic threshold's percentile for this call (None: the model's)

    @property
    def kinds(self):                             # the workspaces the stage visits, first run's first
        return list(dict.fromkeys(run[0] for run in self.runs))

    def state_key(self, T: int):
        """The key of the stage's StageState on its workspace: T for the default call and (T, S, sampler, eta) for a solver, then -- each only
        when it is on -- ("start", a0) for 'dpmpp_2m' (the one table that depends on it), the objective, and "inpaint"."""
        key = T if self.solver is None else (T,) + tuple(self.solver)
        more = ((("start", self.start),) if (self.start and self.solver is not None and self.solver[1] == 'dpmpp_2m') else ()) \
            + (() if self.objective == 'noise' else (self.objective,)) + (() if self.inpaint is None else ("inpaint",))
        return key if not more else (key if isinstance(key, tuple) else (key,)) + more


def graph_key(call: StageCall, cond_scale: float, two: bool, rank, sample0: int, device_noise: bool, group: bool, known: bool,
              rescale: float, sched: bool, length: int = None):
    """The key of a captured graph on its StageState: guidance, threshold rank (k_lo, k_hi, w), shard offset, stage, loop length, noise mode, tail
    kind, then -- each only when it is on -- the solver, "inpaint", ("rescale", phi), "sched", ("len", steps) for a run shorter than the loop, and
    ("thr", mode) for a stage whose x0 is not bounded by the dynamic threshold (a percentile of the call's is in the rank already)."""
    return (float(cond_scale), two, *rank, sample0, call.stage, call.steps, device_noise, group) + (() if call.solver is None else (tuple(call.solver),)) \
        + (("inpaint",) if known else ()) + ((("rescale", rescale),) if rescale else ()) + (("sched",) if sched else ()) \
        + (() if length is None else (("len", length),)) + (() if call.threshold == 'dynamic' else (("thr", call.threshold),))


@dataclasses.dataclass(frozen=True)
class SampleCall:
    """What the stages of one call share.  ``parse`` leaves the tensors where the caller has them; ``placed`` moves them."""
    batch: int
    stages: tuple                                # the StageCalls of the stages that run, in order
    noise: Noise
    use_graph: bool
    precision: str
    lowres_noise_level: float
    texts: Optional[list]                        # captions still to encode (text_embeds None)
    text_embeds: Optional[torch.Tensor]
    text_masks: Optional[torch.Tensor]
    negative: object                             # None, strings still to encode, or (embeds, mask or None)
    inpaint: Optional[tuple]                     # as StageCall.inpaint
    start_image: Optional[torch.Tensor]          # stands in for the output of the stage below the first
    init_images: Optional[torch.Tensor]
    device: Optional[torch.device]
    is_async: bool
    return_pil: bool

    @property
    def tensors(self):                           # every tensor of the caller's that the stage streams read
        return [t for t in (self.text_embeds, self.text_masks, *(self.inpaint or ())[:2], self.start_image, self.init_images,
                            *(self.negative or ())) if torch.is_tensor(t)]

    def placed(self, device, text_embeds, text_masks, negative) -> "SampleCall":
        """The call on ``device``, with its captions encoded."""
        to = lambda t: None if t is None else t.to(device)
        px = lambda t: None if t is None else t.to(device).contiguous()
        inpaint = None if self.inpaint is None else (px(self.inpaint[0]), px(self.inpaint[1]), self.inpaint[2])
        init = px(self.init_images)
        stages = tuple(dataclasses.replace(s, inpaint=s.inpaint and inpaint, init=s.init and (init, s.init[1])) for s in self.stages)
        return dataclasses.replace(self, stages=stages, texts=None, text_embeds=to(text_embeds), text_masks=to(text_masks), inpaint=inpaint, init_images=init,
                                   negative=None if negative is None else tuple(to(t) for t in negative), start_image=px(self.start_image))


def parse_solver(model, sample_steps, sampler, sampler_eta):
    """Per stage: None (the reference's loop on all T timesteps) or (S, sampler, eta).  Host only; raises ValueError on bad values."""
    reject(sampler is not None and sampler not in GaussianDiffusion.SAMPLERS, f"sampler must be one of {GaussianDiffusion.SAMPLERS}, got {sampler!r}")
    name = 'ddpm' if sampler is None else sampler
    if sampler_eta is not None:
        reject(name != 'ddim', "sampler_eta goes with sampler='ddim' only")
        reject(not is_number(sampler_eta) or not 0. <= float(sampler_eta) <= 1., f"sampler_eta must be a number in [0, 1], got {sampler_eta!r}")
    eta = {'ddpm': 1., 'ddim': float(0. if sampler_eta is None else sampler_eta), 'dpmpp_2m': 0.}[name]
    out = []
    for S, sched in zip(per_stage(sample_steps, len(model.unets), "sample_steps"), model.noise_schedulers):
        T = sched.num_timesteps
        S = T if S is None else S
        if isinstance(S, bool) or not isinstance(S, int) or not 2 <= S <= T:
            raise ValueError(f"sample_steps must be an int in [2, {T}] for a stage trained with {T} timesteps, got {S!r}")
        out.append(None if (S == T and name == 'ddpm') else (S, name, eta))
    return out


def parse_inpaint(model, batch_size: int, inpaint_images, inpaint_masks, start_image, start_at_stage, stop_at_stage):
    """-> (first stage, one past the last stage, (images float32 [B, C, H, W], masks uint8 [B, Hm, Wm]) or None, start image float32 or None),
    the tensors still where the caller has them.  Host only; raises ValueError on bad or inconsistent values."""
    n_stages = len(model.unets)

    def stage_index(v, name, lo, hi):
        reject(isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi, f"{name} must be an int in [{lo}, {hi}] for a cascade of {n_stages} stages, got {v!r}")
        return v

    stop = n_stages if stop_at_stage is None else stage_index(stop_at_stage, "stop_at_stage", 1, n_stages)
    start = 0
    reject((start_image is None) != (start_at_stage is None), "start_image and start_at_stage go together")
    if start_at_stage is not None:
        start = stage_index(start_at_stage, "start_at_stage", 1, n_stages - 1)
        reject(start >= stop, f"start_at_stage = {start} must be below stop_at_stage = {stop}")
        reject(not model.unets[start].lowres_cond, f"stage {start} takes no low-resolution conditioning image: it cannot start from one")
        start_image = pixel_images(start_image, "start_image", batch_size, model.channels)
    inpaint = None
    reject((inpaint_images is None) != (inpaint_masks is None), "inpaint_images and inpaint_masks go together")
    if inpaint_images is not None:
        inpaint_images = pixel_images(inpaint_images, "inpaint_images", batch_size, model.channels)
        m = inpaint_masks
        reject(not torch.is_tensor(m) or m.dim() not in (3, 4) or (m.dim() == 4 and m.shape[1] != 1), "inpaint_masks must be a tensor [B, H, W] or [B, 1, H, W]")
        reject(m.shape[0] != batch_size, f"inpaint_masks: batch {m.shape[0]} does not match the text batch {batch_size}")
        m = m.detach().reshape(m.shape[0], m.shape[-2], m.shape[-1])
        reject(m.shape[1] < 1 or m.shape[2] < 1, "inpaint_masks: empty")
        reject(m.dtype != torch.bool and not bool(((m == 0) | (m == 1)).all()), "inpaint_masks must hold 0 / 1 (or be bool)")
        inpaint = (inpaint_images, m.to(torch.uint8))
    return start, stop, inpaint, start_image


def parse_init(model, batch_size: int, init_images, init_strength, solvers, first_stage: int, end_stage: int):
    """-> (init images float32 [B, C, H, W] still where the caller has them, or None; per stage None -- the stage starts from pure noise -- or a0, the number
    of loop steps it skips: init_start_step).  A strength for a stage the call does not run is ignored.  Host only; raises ValueError on bad values."""
    n_stages = len(model.unets)
    reject((init_images is None) != (init_strength is None), "init_images and init_strength go together")
    if init_images is None:
        return None, [None] * n_stages
    images = pixel_images(init_images, "init_images", batch_size, model.channels)
    if not isinstance(init_strength, (list, tuple)) and not is_number(init_strength):
        raise ValueError(f"init_strength must be a number in (0, 1] or a list with a number or None per stage, got {init_strength!r}")
    starts = [None] * n_stages
    for stage, v in enumerate(per_stage(init_strength, n_stages, "init_strength", noun="entry")):
        if v is None:
            continue
        n_steps = model.noise_schedulers[stage].num_timesteps if solvers[stage] is None else solvers[stage][0]
        a0 = init_start_step(n_steps, v)                     # (validates the value of every entry, run or not)
        if first_stage <= stage < end_stage:
            starts[stage] = a0
    reject(all(a0 is None for a0 in starts), "init_strength: every stage the call runs has None")
    return images, starts


def parse_guidance(model, batch_size: int, cond_scale, texts, text_embeds, text_masks, negative_texts, negative_text_embeds,
                   negative_text_masks, guidance_rescale, guided: bool = None):
    """``guided``: whether any step of the call is guided (None: ``cond_scale`` != 1, a call without a guidance schedule).  -> (phi: 0. when off, negative
    captions: None, a list of ``batch_size`` strings, or (embeds, mask or None) still where the caller has them).  Host only; raises ValueError on bad values."""
    phi = 0.
    if guidance_rescale is not None:
        reject(not is_number(guidance_rescale) or not 0. <= float(guidance_rescale) <= 1., f"guidance_rescale must be a number in [0, 1], got {guidance_rescale!r}")
        phi = float(guidance_rescale)
    negative = None
    reject(negative_texts is not None and negative_text_embeds is not None, "pass negative_texts or negative_text_embeds, not both")
    reject(negative_text_masks is not None and negative_text_embeds is None, "negative_text_masks goes with negative_text_embeds")
    masked = text_masks is not None or text_embeds is None                # (captions encoded here always come with masks)
    if negative_texts is not None:
        if isinstance(negative_texts, str):
            negative_texts = [negative_texts] * batch_size
        if not isinstance(negative_texts, (list, tuple)) or not all(isinstance(t, str) for t in negative_texts):
            raise ValueError("negative_texts must be a string or a list of strings")
        reject(len(negative_texts) != batch_size, f"negative_texts: batch {len(negative_texts)} does not match the text batch {batch_size}")
        reject(not masked, "negative_texts are encoded with masks: pass text_masks with text_embeds (the captions and the negative captions "
                           "must both carry masks, or neither)")
        negative = list(negative_texts)
    elif negative_text_embeds is not None:
        e, m = negative_text_embeds, negative_text_masks
        reject(not torch.is_tensor(e) or e.dim() != 3 or not e.is_floating_point(), "negative_text_embeds must be a float tensor [B, L, E]")
        reject(e.shape[0] != batch_size, f"negative_text_embeds: batch {e.shape[0]} does not match the text batch {batch_size}")
        reject(e.shape[2] != model.text_embed_dim, f"negative_text_embeds: embedding dimension {e.shape[2]}, the model has {model.text_embed_dim}")
        if m is not None and (not torch.is_tensor(m) or tuple(m.shape) != tuple(e.shape[:2])):
            raise ValueError(f"negative_text_masks must be a tensor {tuple(e.shape[:2])} like negative_text_embeds")
        reject(masked != (m is not None), "negative prompts: the captions and the negative captions must both carry masks, or neither")
        reject(m is None and text_embeds is not None and text_embeds.shape[1] != e.shape[1],
               f"negative prompts: unmasked captions of different lengths ({text_embeds.shape[1]} and {e.shape[1]}) cannot be joined; pass masks")
        negative = (e.detach(), None if m is None else m.detach())
    reject((phi or negative is not None) and not (cond_scale != 1. if guided is None else guided), "negative prompts and guidance_rescale need "
           "cond_scale != 1 (or a guidance schedule with a guided step): at 1 the second half of the guidance batch is never evaluated")
    return phi, negative


def parse_guidance_schedule(model, batch_size: int, cond_scale, solvers, guidance_interval, guidance_schedule):
    """-> None when neither keyword is given, else per stage None (``cond_scale`` on every step, the call as it was) or that stage's guidance
    scales, float64 [S] or [S, B] in execution order (guidance_scale_table).  Host only; raises ValueError on bad values."""
    if guidance_interval is None and guidance_schedule is None:
        return None
    n_stages = len(model.unets)
    intervals = [None] * n_stages
    if guidance_interval is not None:
        is_pair = lambda v: isinstance(v, (list, tuple)) and len(v) == 2 and all(is_number(x) for x in v)
        intervals = per_stage(guidance_interval, n_stages, "guidance_interval", is_pair, noun="entry", counted=False)
        for iv in intervals:
            reject(iv is not None and (not is_pair(iv) or not 0. <= float(iv[0]) <= float(iv[1]) <= 1.),
                   f"guidance_interval must be (lo, hi) with 0 <= lo <= hi <= 1 (or None for a stage), got {iv!r}")
        reject(all(iv is None for iv in intervals), "guidance_interval: every stage's entry is None")
        intervals = [None if iv is None else (float(iv[0]), float(iv[1])) for iv in intervals]
    schedules = [None] * n_stages
    if guidance_schedule is not None:
        reject(cond_scale != 1., "guidance_schedule is the scale itself: leave cond_scale at 1")
        schedules = per_stage(guidance_schedule, n_stages, "guidance_schedule", callable, noun="entry", counted=False)
        reject(all(s is None for s in schedules), "guidance_schedule: every stage's entry is None")
    elif cond_scale == 1.:
        raise ValueError("guidance_interval needs cond_scale != 1 (or a guidance_schedule): outside the interval the scale is 1 already")
    reject(not is_number(cond_scale) or cond_scale != cond_scale or abs(cond_scale) == float("inf"), f"cond_scale must be a finite number, got {cond_scale!r}")
    tables = []
    for stage, sched in enumerate(model.noise_schedulers):
        if intervals[stage] is None and schedules[stage] is None:
            tables.append(None)
            continue
        T = sched.num_timesteps
        tau = torch.arange(T) if solvers[stage] is None else sched.sampling_timestep_map(solvers[stage][0])
        tables.append(guidance_scale_table(tau, T, batch_size, cond_scale, intervals[stage], schedules[stage]))
    return tables


THRESHOLDING = ('dynamic', 'static', 'none')


def parse_thresholding(model, thresholding, thresholding_percentile, first_stage: int, end_stage: int):
    """-> per stage (mode, percentile or None: the model's).  ``thresholding``: one of THRESHOLDING for every stage, or a list / tuple with one per
    stage (None there: 'dynamic'); ``thresholding_percentile``: None, a number in [0, 1] for every stage, or a list / tuple with a number or None
    per stage -- for 'dynamic' stages only.  Every entry's value is validated; a percentile on a 'static' / 'none' stage the call does not run is
    ignored.  Host only; raises ValueError on bad values."""
    n_stages = len(model.unets)
    modes = ['dynamic' if m is None else m for m in per_stage(thresholding, n_stages, "thresholding")]
    for m in modes:
        reject(not isinstance(m, str) or m not in THRESHOLDING, f"thresholding must be one of {THRESHOLDING} (or None in a list: 'dynamic'), got {m!r}")
    pcts = per_stage(thresholding_percentile, n_stages, "thresholding_percentile", noun="entry")
    for p in pcts:
        reject(p is not None and (not is_number(p) or not 0. <= float(p) <= 1.),
               f"thresholding_percentile must be a number in [0, 1] (or None), got {p!r}")
    for stage in range(first_stage, end_stage):
        reject(pcts[stage] is not None and modes[stage] != 'dynamic',
               f"thresholding_percentile goes with thresholding='dynamic' only: stage {stage} is {modes[stage]!r}")
    return [(m, None if p is None else float(p)) for m, p in zip(modes, pcts)]


def parse(model, *, texts, text_masks, text_embeds, cond_scale, lowres_sample_noise_level, return_pil_images, device, _noise, _seed,
          _sample_offset, _use_graph, _precision, _async, sample_steps, sampler, sampler_eta, inpaint_images, inpaint_masks, start_image,
          start_at_stage, stop_at_stage, negative_texts, negative_text_embeds, negative_text_masks, guidance_rescale, guidance_interval,
          guidance_schedule, init_images, init_strength, thresholding, thresholding_percentile) -> SampleCall:
    """Every keyword of ``Imagen.sample()`` (all of them, by name: one that is not listed here is a TypeError, never silently dropped) -> the SampleCall.  Host work
    only, so every ValueError -- and the assertions on the captions and on guidance without conditional dropout -- is raised before anything is launched."""
    solvers = parse_solver(model, sample_steps, sampler, sampler_eta)
    assert text_embeds is not None or texts is not None, 'text or text encodings must be passed into Imagen'
    n_rows = text_embeds.shape[0] if text_embeds is not None else len(texts)
    first_stage, end_stage, inpaint, start_image = parse_inpaint(model, n_rows, inpaint_images, inpaint_masks, start_image, start_at_stage, stop_at_stage)
    init_images, init_starts = parse_init(model, n_rows, init_images, init_strength, solvers, first_stage, end_stage)
    thresholds = parse_thresholding(model, thresholding, thresholding_percentile, first_stage, end_stage)
    scale_tabs = parse_guidance_schedule(model, n_rows, cond_scale, solvers, guidance_interval, guidance_schedule)
    guided = None
    if scale_tabs is not None:                               # (of the steps a stage executes: a loop that starts at an init image skips its first ones)
        guided = any(cond_scale != 1. if scale_tabs[s] is None else bool((scale_tabs[s][init_starts[s] or 0:] != 1.).any())
                     for s in range(first_stage, end_stage))
    rescale, negative = parse_guidance(model, n_rows, cond_scale, texts, text_embeds, text_masks, negative_texts, negative_text_embeds,
                                       negative_text_masks, guidance_rescale, guided)
    assert text_embeds is None or text_embeds.shape[-1] == model.text_embed_dim, \
        f'invalid text embedding dimension being passed in (should be {model.text_embed_dim})'
    normalize = model.auto_normalize_img
    inpaint = inpaint and inpaint + (normalize,)
    stages = []
    for stage in range(first_stage, end_stage):
        n_steps = model.noise_schedulers[stage].num_timesteps if solvers[stage] is None else solvers[stage][0]
        a0 = init_starts[stage] or 0                         # a stage that starts from an init image: the plan of the steps [a0, S) it executes
        w_stage = None if scale_tabs is None else scale_tabs[stage]
        # ONE run over all steps for a call without a schedule or interval -- and for a table that is one row-uniform value on every step,
        # which IS that call (guidance_plan)
        runs = [('plain' if cond_scale == 1. else 'scalar', a0, n_steps, cond_scale)] if w_stage is None else \
            [(kind, a + a0, b + a0, scale) for kind, a, b, scale in guidance_plan(w_stage[a0:])]
        stages.append(StageCall(stage, n_steps, solvers[stage], a0, model.pred_objectives[stage], inpaint,
                                None if init_starts[stage] is None else (init_images, normalize), tuple(runs), w_stage, rescale, *thresholds[stage]))
    assert model.can_classifier_guidance or all(kind == 'plain' for s in stages for kind, *_ in s.runs), \
        'imagen was not trained with conditional dropout, and thus one cannot use classifier free guidance (cond_scale anything other than 1)'
    return SampleCall(
        batch=n_rows, stages=tuple(stages), noise=Noise(_noise, _seed, _sample_offset), use_graph=_use_graph,
        precision=_precision if _precision is not None else os.environ.get("MINIMAGEN_PRECISION", "fp32"),
        lowres_noise_level=model.lowres_sample_noise_level if lowres_sample_noise_level is None else lowres_sample_noise_level,
        texts=texts if text_embeds is None else None, text_embeds=text_embeds, text_masks=text_masks, negative=negative, inpaint=inpaint,
        start_image=start_image, init_images=init_images, device=device, is_async=_async, return_pil=return_pil_images)
