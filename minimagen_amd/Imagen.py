"""``Imagen`` with the reference's constructor and ``sample`` API (minimagen/Imagen.py), whose cascaded
reverse-diffusion loop runs as HIP kernels replayed from a HIP graph on MI355X."""
from __future__ import annotations

import os
from typing import Callable, List, Literal, Tuple, Union

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib as L
from . import sample_call
from . import sampler as S
from . import train_ops
from .Unet import Unet
from .diffusion_model import GaussianDiffusion
from .helpers import (cast_tuple, default, eval_decorator, exists, module_device, normalize_neg_one_to_one, null_context, resize_image_to)
from .sample_call import SampleCall, StageCall
from .t5 import get_encoded_dim, t5_encode_text

# the sampler tail of images too large for one workgroup (the super-resolution stages) as ONE launch of cooperating workgroups
# (mi_sampler_step_group_fwd) instead of five launches; 0: the separate kernels
SAMPLER_GROUP = int(os.environ.get("MINIMAGEN_SAMPLER_GROUP", "1"))
# ... for at most this many workgroups per image (8: up to 256^2).  The workgroups of an image wait for each other, so a launch is only safe
# next to OTHER launches of the same kind while the partial groups of all of them fit the chip beside everything else that is resident: two
# 1024^2 tails (128 workgroups of 1024 work-items per image, one per CU) in flight on two call lanes starved each other's last image until the
# bounded spin gave up (profiles/r04_sampler_group_config5.txt) -- large images keep the separate kernels
SAMPLER_GROUP_MAX = int(os.environ.get("MINIMAGEN_SAMPLER_GROUP_MAX", "8"))
# sampler stage states kept per workspace for calls with sample_steps / sampler / sampler_eta (one per (T, S, sampler, eta): coefficient
# table, step tables of S x B2 rows, history buffer, up to 8 graphs); the least recently used one goes when a new setting arrives
MAX_SOLVER_STATES = max(1, int(os.environ.get("MINIMAGEN_SOLVER_STATES", "8")))
SAMPLE_LANES = max(1, int(os.environ.get("MINIMAGEN_SAMPLE_LANES", "2")))     # independent call lanes of sample(_async=True)
# 1: a synchronous sample() waits on the HOST for its last stage and checks the cooperative kernels' status words before it returns (the
# default defers the check to the next API entry: the failed call's images are NaN -- fail-stop -- so nothing plausible-but-wrong escapes)
STRICT_STATUS = os.environ.get("MINIMAGEN_STRICT_STATUS", "0") != "0"
_STAGE_STREAMS = {}          # (device, lanes, stages, priority mode) -> [lane][stage] HIP streams, process-wide (see Imagen._call_streams)


class Imagen(nn.Module):
    """minimagen/Imagen.py:22-131."""

    def __init__(
            self,
            unets: Union[Unet, List[Unet], Tuple[Unet, ...]],
            *,
            text_encoder_name: str,
            image_sizes: Union[int, List[int], Tuple[int, ...]],
            text_embed_dim: int = None,
            channels: int = 3,
            timesteps: Union[int, List[int], Tuple[int, ...]] = 1000,
            cond_drop_prob: float = 0.1,
            loss_type: Literal["l1", "l2", "huber"] = 'l2',
            lowres_sample_noise_level: float = 0.2,
            auto_normalize_img: bool = True,
            dynamic_thresholding_percentile: float = 0.9,
            only_train_unet_number: int = None,
            pred_objectives: Union[str, List[str], Tuple[str, ...]] = 'noise',
            min_snr_loss_weight: Union[bool, List[bool], Tuple[bool, ...]] = False,
            min_snr_gamma: Union[float, List[float], Tuple[float, ...]] = 5.
    ):
        """Not in the reference (keyword-only, one value or one per U-Net): ``pred_objectives`` = what each U-Net predicts and
        is trained on -- 'noise' (the reference's), 'x_start' or 'v' (Salimans & Ho 2022: sqrt(abar) eps - sqrt(1 - abar) x0);
        ``min_snr_loss_weight`` with ``min_snr_gamma`` > 0: the min-SNR-gamma loss weight per timestep (Hang et al. 2023;
        GaussianDiffusion.loss_weight_table).  Bad values raise ValueError.  The defaults are the reference's training and sampling."""
        super().__init__()
        if loss_type not in ('l1', 'l2', 'huber'):
            raise NotImplementedError()
        self.loss_type = loss_type
        self.channels = channels
        unets = cast_tuple(unets)
        num_unets = len(unets)

        def per_unet(val, name, ok, what):
            vals = tuple(sample_call.per_stage(val, num_unets, name, unit="U-Net"))
            for v in vals:
                sample_call.reject(not ok(v), f"{name} must be {what}, got {v!r}")
            return vals
        self.pred_objectives = per_unet(pred_objectives, "pred_objectives", lambda v: isinstance(v, str) and v in GaussianDiffusion.OBJECTIVES,
                                        f"one of {GaussianDiffusion.OBJECTIVES}")
        self.min_snr_loss_weight = per_unet(min_snr_loss_weight, "min_snr_loss_weight", lambda v: isinstance(v, bool), "a bool")
        self.min_snr_gamma = tuple(float(v) for v in per_unet(
            min_snr_gamma, "min_snr_gamma", lambda v: sample_call.is_number(v) and v > 0. and v == v, "a positive number"))
        self._loss_weights = {}                  # (U-Net index, device) -> the fp32 weight table of that U-Net's min-SNR setting, where the loss reads it
        self.noise_schedulers = nn.ModuleList([GaussianDiffusion(timesteps=t) for t in cast_tuple(timesteps, num_unets)])
        # built from the RAW argument like Imagen.py:78 (so only an int works, as in the reference)
        self.lowres_noise_schedule = GaussianDiffusion(timesteps=timesteps)
        self.text_encoder_name = text_encoder_name
        self.text_embed_dim = default(text_embed_dim, lambda: get_encoded_dim(text_encoder_name))
        self.unet_being_trained_index = -1
        self.only_train_unet_number = only_train_unet_number
        self.unets = nn.ModuleList([])
        for ind, one_unet in enumerate(unets):
            assert isinstance(one_unet, Unet)
            one_unet = one_unet._cast_model_parameters(lowres_cond=not ind == 0, text_embed_dim=self.text_embed_dim,
                                                       channels=self.channels, channels_out=self.channels)
            self.unets.append(one_unet)
        self.image_sizes = cast_tuple(image_sizes)
        assert num_unets == len(image_sizes), f'you did not supply the correct number of u-nets ({len(self.unets)}) for resolutions {image_sizes}'
        self.sample_channels = cast_tuple(self.channels, num_unets)
        self.lowres_sample_noise_level = lowres_sample_noise_level
        self.cond_drop_prob = cond_drop_prob
        self.can_classifier_guidance = cond_drop_prob > 0.
        self.auto_normalize_img = auto_normalize_img
        self.input_image_range = (0. if auto_normalize_img else -1., 1.)
        self.dynamic_thresholding_percentile = dynamic_thresholding_percentile
        self.register_buffer('_temp', torch.tensor([0.]), persistent=False)
        self.to(next(self.unets.parameters()).device)
        self._status_stages, self._status_pending, self._lane_done = [], [], {}      # see _poll_status / wait_pending_samples

    @property
    def device(self) -> torch.device:
        return self._temp.device

    def _reset_unets_all_one_device(self, device: torch.device = None):
        """Imagen.py:205-219.  All U-Nets stay resident on the GPU (288 GB of HBM: nothing is swapped to the host)."""
        device = default(device, self.device)
        self.unets = nn.ModuleList([*self.unets])
        self.unets.to(device)
        self.unet_being_trained_index = -1

    def state_dict(self, *args, **kwargs):
        self._reset_unets_all_one_device()
        return super().state_dict(*args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        self._reset_unets_all_one_device()
        return super().load_state_dict(*args, **kwargs)

    # ------------------------------------------------------------------ training (Imagen.py:512-650)
    def _get_unet(self, unet_number: int) -> Unet:
        """Imagen.py:221-259.  All U-Nets stay on the GPU (288 GB of HBM); only the bookkeeping of the reference is kept."""
        assert 0 < unet_number <= len(self.unets)
        self.unet_being_trained_index = unet_number - 1
        return self.unets[unet_number - 1]

    def _p_losses(self, unet: Unet, x_start, times, *, noise_scheduler: GaussianDiffusion, lowres_cond_img=None, lowres_aug_times=None,
                  text_embeds=None, text_mask=None, noise=None, unet_index: int = None):
        """Imagen.py:512-573: corrupt x_0 with q_sample, predict the noise, loss against the true noise.  A U-Net with another objective or with
        the min-SNR weight (``unet_index``: which one, default the one _get_unet handed out last) goes through train_ops.diffuse /
        train_ops.objective_loss: same draws in the same order, the target and the weighted loss of DESIGN.md section 20."""
        k = default(unet_index, max(self.unet_being_trained_index, 0))
        objective, weighted = self.pred_objectives[k], self.min_snr_loss_weight[k]
        noise = default(noise, lambda: torch.randn_like(x_start))
        if objective != 'noise' or weighted:
            x_noisy, target = train_ops.diffuse(x_start, noise, times, noise_scheduler, normalize=self.auto_normalize_img, target=objective)
            lowres_noisy = None
            if exists(lowres_cond_img):
                lowres_aug_times = default(lowres_aug_times, times)
                lowres_noisy, _ = train_ops.diffuse(lowres_cond_img, torch.randn_like(lowres_cond_img), lowres_aug_times, self.lowres_noise_schedule,
                                                    normalize=self.auto_normalize_img, target=None)
            pred = unet.forward(x_noisy, times, text_embeds=text_embeds, text_mask=text_mask, lowres_noise_times=lowres_aug_times,
                                lowres_cond_img=lowres_noisy, cond_drop_prob=self.cond_drop_prob)
            weights = None
            if weighted:
                weights = self._loss_weights.get((k, pred.device))
                if weights is None:
                    weights = self._loss_weights[(k, pred.device)] = noise_scheduler.loss_weight_table(objective, self.min_snr_gamma[k]).to(pred.device)
            return train_ops.objective_loss(pred, target, times, weights, self.loss_type)
        norm = normalize_neg_one_to_one if self.auto_normalize_img else (lambda v: v)
        x_start = norm(x_start)
        x_noisy = noise_scheduler.q_sample(x_start=x_start, t=times, noise=noise)
        lowres_noisy = None
        if exists(lowres_cond_img):
            lowres_aug_times = default(lowres_aug_times, times)
            lowres_cond_img = norm(lowres_cond_img)
            lowres_noisy = self.lowres_noise_schedule.q_sample(x_start=lowres_cond_img, t=lowres_aug_times, noise=torch.randn_like(lowres_cond_img))
        pred = unet.forward(x_noisy, times, text_embeds=text_embeds, text_mask=text_mask, lowres_noise_times=lowres_aug_times,
                            lowres_cond_img=lowres_noisy, cond_drop_prob=self.cond_drop_prob)
        return {'l1': F.l1_loss, 'l2': F.mse_loss, 'huber': F.smooth_l1_loss}[self.loss_type](pred, noise)

    def forward(self, images, texts: List[str] = None, text_embeds: torch.Tensor = None, text_masks: torch.Tensor = None, unet_number: int = None):
        """Imagen.py:575-650: the training loss of ONE U-Net of the cascade on a batch of images + captions.  The U-Net runs through its
        differentiable training graph when it is in train mode with autograd on (Unet._forward_train: HIP kernels for the convolution stack,
        forward and backward, torch ops for the rest -- minimagen_amd/train_ops.py) and through the HIP inference engine otherwise
        (evaluation of the loss)."""
        assert not (len(self.unets) > 1 and not exists(unet_number)), \
            f'you must specify which unet you want trained, from a range of 1 to {len(self.unets)}, if you are training cascading DDPM (multiple unets)'
        unet_number = default(unet_number, 1)
        assert not exists(self.only_train_unet_number) or self.only_train_unet_number == unet_number, \
            f'you can only train on unet #{self.only_train_unet_number}'
        k = unet_number - 1
        unet, noise_scheduler, target = self._get_unet(unet_number), self.noise_schedulers[k], self.image_sizes[k]
        prev = self.image_sizes[k - 1] if k > 0 else None
        assert images.dim() == 4 and images.shape[1] == self.channels, f'images must be (b, {self.channels}, h, w)'
        b, _, h, w = images.shape
        assert h >= target and w >= target
        times = noise_scheduler._sample_random_times(b, device=images.device)
        if exists(texts) and not exists(text_embeds):
            assert len(texts) == len(images), 'number of text captions does not match up with the number of images given'
            text_embeds, text_masks = t5_encode_text(texts, name=self.text_encoder_name)
            text_embeds, text_masks = text_embeds.to(images.device), text_masks.to(images.device)
        assert exists(text_embeds), 'text or text encodings must be passed into decoder'
        assert text_embeds.shape[-1] == self.text_embed_dim, f'invalid text embedding dimension being passed in (should be {self.text_embed_dim})'
        lowres_cond_img = lowres_aug_times = None
        if exists(prev):
            lowres_cond_img = resize_image_to(images, prev, clamp_range=self.input_image_range, pad_mode='reflect')
            lowres_cond_img = resize_image_to(lowres_cond_img, target, clamp_range=self.input_image_range, pad_mode='reflect')
            lowres_aug_times = self.lowres_noise_schedule._sample_random_times(1, device=images.device).expand(b)
        images = resize_image_to(images, target)
        return self._p_losses(unet, images, times, text_embeds=text_embeds, text_mask=text_masks, noise_scheduler=noise_scheduler,
                              lowres_cond_img=lowres_cond_img, lowres_aug_times=lowres_aug_times, unet_index=k)

    # ------------------------------------------------------------------ sampling (the loop itself: minimagen_amd/sampler.py)
    def _stage_state(self, ws, sched: GaussianDiffusion, shape, call: StageCall, eng=None):
        return S.stage_state(ws, sched, shape, call, eng, MAX_SOLVER_STATES)

    def _stage_begin(self, unet: Unet, shape, ws, call: StageCall, **kw):          # -> (stage state, injected noise)
        return S.stage_begin(unet, shape, ws, call, max_states=MAX_SOLVER_STATES, **kw)

    def _p_sample_loop(self, unet: Unet, shape, ws, call: StageCall, run=None, **kw):        # Imagen.py:373-420 -> the stage's image
        return S.p_sample_loop(self, unet, shape, ws, call, run, group_max=SAMPLER_GROUP_MAX if SAMPLER_GROUP else 0, max_states=MAX_SOLVER_STATES, **kw)

    _parse_solver, _parse_inpaint, _parse_init = sample_call.parse_solver, sample_call.parse_inpaint, sample_call.parse_init         # (host: sample_call.py)
    _parse_guidance, _parse_guidance_schedule = sample_call.parse_guidance, sample_call.parse_guidance_schedule
    _parse_thresholding = sample_call.parse_thresholding

    def _lowres_conditioning(self, unet: Unet, img, image_size: int, ws, lowres_noise_level: float, noise_fn, seed, sample0, stage):
        """Imagen.py:479-485 + :393: cubic resize (reflect pad) -> q_sample at int(T*level) -> *2-1."""
        lib = L.lib()
        stream = L.current_stream()
        B, Cc, Hin, Win = img.shape
        t_low = int(self.lowres_noise_schedule.num_timesteps * lowres_noise_level)          # diffusion_model.py:68-69
        ws.lowres_times.fill_(t_low)
        up = S.cubic_resize(ws, img, image_size, stream)
        n = Cc * image_size * image_size
        if noise_fn is not None:
            noise = noise_fn(up.shape).to(ws.dev).contiguous()                  # Imagen.py:485 randn_like
        else:
            noise = torch.empty_like(up)
            L.check(lib.mi_randn_fill(L.ptr(noise), B, n, seed, sample0, (stage << 20) | (1 << 19), stream), "mi_randn_fill")
        a = self.lowres_noise_schedule._host_sqrt_alphas_cumprod[t_low]
        b = self.lowres_noise_schedule._host_sqrt_one_minus_alphas_cumprod[t_low]
        L.check(lib.mi_lowres_augment(L.ptr(up), L.ptr(noise), L.ptr(ws.lowres), B * n, a, b, 1 if self.auto_normalize_img else 0, stream), "mi_lowres_augment")
        ws.lowres_keepalive = (up, noise)
        unet.engine().prepare_lowres(ws, stream)

    @torch.no_grad()
    @eval_decorator
    def sample(self, texts: List[str] = None, text_masks: torch.Tensor = None, text_embeds: torch.Tensor = None,
               cond_scale: float = 1., lowres_sample_noise_level: float = None, return_pil_images: bool = False,
               device: torch.device = None, *, _noise: Callable = None, _seed: int = 1234, _sample_offset: int = 0,
               _use_graph: bool = True, _precision: str = None, _async: bool = False,
               sample_steps: Union[int, List[int], Tuple[int, ...]] = None, sampler: str = None, sampler_eta: float = None,
               inpaint_images: torch.Tensor = None, inpaint_masks: torch.Tensor = None, start_image: torch.Tensor = None,
               start_at_stage: int = None, stop_at_stage: int = None,
               negative_texts: Union[str, List[str]] = None, negative_text_embeds: torch.Tensor = None, negative_text_masks: torch.Tensor = None,
               guidance_rescale: float = None, guidance_interval=None, guidance_schedule=None,
               init_images: torch.Tensor = None, init_strength=None, thresholding='dynamic', thresholding_percentile=None):
        """minimagen/Imagen.py:424-510.  Private keyword-only extras (not in the reference): ``_noise(shape)`` injects a
        host noise stream in the reference's draw order (parity runs); otherwise noise is Philox keyed by
        (``_seed``, ``_sample_offset`` + row, stage, step, element) so a sharded batch reproduces the unsharded one;
        ``_precision`` = "fp32" (default) or "half" (single-fp16-term matrix-core contractions, see engine.UnetEngine.precision);
        ``_async=True`` returns without making the caller's stream wait (``self.last_sample_done`` / the returned tensor's ``sample_done`` is THIS call's completion event; ``wait_pending_samples()`` covers every lane): successive
        calls then pipeline across the per-stage streams (the base stage of the next batch under the super-resolution stage of this one).

        Sampling in fewer steps (keyword-only, not in the reference): ``sample_steps`` = S, an int or one int per stage, 2 <= S <= T of
        that stage's schedule (None: T) walks S of the trained timesteps, tau_k = round(k (T-1) / (S-1)), one U-Net evaluation each.
        ``sampler`` = 'ddpm' (default: the reference's ancestral step on the subsequence), 'ddim' (eta = ``sampler_eta``, default 0) or
        'dpmpp_2m' (DPM-Solver++ 2M on the thresholded x0, deterministic); ``sampler_eta`` in [0, 1] goes with 'ddim' only.  S = T with
        'ddpm' IS the reference's loop.  Tables: GaussianDiffusion.sampler_tables.

        Conditioning on pixels the caller has (keyword-only, not in the reference).  ``inpaint_images`` ([B, C, H, W]
        float in [0, 1], square, any size) with ``inpaint_masks`` ([B, H, W] or [B, 1, H, W], bool or 0/1, nonzero = "known, keep"): every
        stage re-imposes the known pixels -- the images resized to its size (cubic, antialiased when shrinking), the masks by nearest
        neighbour -- at the noise level of EVERY step, inside the sampler tails, for every ``sampler`` / ``sample_steps``; the returned
        images carry them.  One pass per step: no RePaint resampling.  ``start_image`` ([B, C, H, W] in [0, 1], square, any size) with
        ``start_at_stage`` = s >= 1 skips the stages below s and stands in for the output of stage s - 1 (run only the super-resolution
        stage on an image of the caller's); ``stop_at_stage`` = s runs the stages below s and returns that stage's image.  The noise is
        keyed by the stage INDEX, so a cascade cut in two this way gives the bits of the whole.

        A stage whose U-Net was built with ``pred_objectives`` 'v' or 'x_start' samples from a coefficient table whose columns 0 and 1 turn
        that prediction into x0 (GaussianDiffusion.sampler_coef_table), for every setting above; nothing else differs, and a 'noise' stage is
        untouched.

        More of classifier-free guidance (keyword-only, not in the reference; both need ``cond_scale`` != 1).  Negative
        prompts: ``negative_texts`` (B strings, or one for every row; encoded like ``texts``) or ``negative_text_embeds`` [B, Ln, E] with an
        optional ``negative_text_masks`` [B, Ln] -- the rows of the guidance batch that see the learned null embeddings otherwise are
        conditioned on that caption, and the result is neg + (pos - neg) * cond_scale.  Ln may differ from the captions' length only when
        both sides carry masks (the shorter is padded with zero embeddings under a False mask); both sides masked, or neither.
        ``guidance_rescale`` = phi in [0, 1] (Lin et al. 2023; None and 0: off): per image, the guided prediction g is scaled to the standard
        deviation of the conditional prediction c and mixed with itself, g * (phi * std(c) / std(g) + 1 - phi), on what the U-Net predicts
        (whatever its objective), before x0 and the dynamic threshold.  Both go with every setting above.  Nothing here has been tried on a
        trained model: what is checked is the arithmetic.

        Guidance over the steps (keyword-only, not in the reference).  ``guidance_interval`` = (lo, hi), 0 <= lo <= hi <= 1,
        one pair for every stage or a list with a pair or None per stage (needs ``cond_scale`` != 1 or a schedule): the step at trained
        timestep tau is guided with ``cond_scale`` iff lo (T - 1) <= tau <= hi (T - 1) (Kynkaanniemi et al. 2024); every other step runs
        unguided, over B rows of the U-Net instead of 2 B.  ``guidance_schedule`` IS the scale per step (``cond_scale`` stays 1): a callable
        f(u) -> float of u = tau / (T - 1) for every stage, or a list with one entry per stage -- None, a callable, or a float tensor /
        sequence [S] or [S, B] (per row), entry 0 the first step executed (the noisiest).  With both, steps outside the interval get scale 1.
        A step whose scales are all exactly 1 is unguided (negative prompts and ``guidance_rescale``, the identity there, are skipped; they
        need one guided step somewhere).  A stage moves between its B-row and its 2 B-row workspace at the run boundaries (x, the
        dpmpp_2m history and the step index are handed over; same noise stream); an interval of (0, 1), a constant schedule s or an
        all-ones schedule IS the call with ``cond_scale`` = s / 1.

        Starting from an image (SDEdit / "img2img"; keyword-only, not in the reference).  ``init_images`` ([B, C, H, W]
        float in [0, 1], square, any size; resized per stage like ``inpaint_images``) with ``init_strength`` = s in (0, 1] for every stage, or
        a list with s or None (that stage starts from pure noise, as without the keywords) per stage: a stage of S loop steps skips its
        first a0 = S - m, m = min(S, max(1, floor(s S + 0.5))) (sample_call.init_start_step), and runs the other m from
        x = sqrt(abar_tau) y' + sqrt(1 - abar_tau) eps at tau = the trained timestep of step a0 (GaussianDiffusion.init_start_coefs) -- eps IS
        the stage's own x_T draw and every other draw keeps its index in the full loop, so a sharded batch reproduces the unsharded one and
        ``_noise`` is called in the order it is called today.  With every ``sampler`` / ``sample_steps`` ('dpmpp_2m': the first executed
        step is first order), with inpainting (blend 0 at the starting level), with ``start_image`` / ``start_at_stage`` / ``stop_at_stage`` (a
        strength for a stage that does not run is ignored) and with the guidance keywords, whose intervals and schedules stay indexed by the
        step of the FULL loop ([S] / [S, B] keep their shape, entry a0 is the first one executed; "one guided step somewhere" means an
        executed one).  One strength per stage, not per row; no RePaint resampling.  Nothing here has been tried on a trained model:
        what is checked is the arithmetic.

        How x0 is bounded (keyword-only, not in the reference).  ``thresholding`` = 'dynamic' (default: the reference's
        x0 = clamp(x0, -s, s) / s with s = max(1, the per-image quantile of |x0|)), 'static' (x0 = clamp(x0, -1, 1), the baseline of the Imagen
        paper; a NaN stays NaN) or 'none' (x0 as predicted: what exact DDIM needs) -- one value for every stage, or a list / tuple with one per
        stage (None there: 'dynamic').  ``thresholding_percentile`` = a number in [0, 1] for every stage, or a list with a number or None per
        stage, stands in for ``dynamic_thresholding_percentile`` for this call; only for stages whose mode is 'dynamic' (ValueError for a stage
        that runs with 'static' or 'none').  Everything behind x0 -- the posterior or solver step, the 'dpmpp_2m' history, the draw, the
        inpainting blend, the final clamp to [-1, 1] of the image -- sees the x0 of the chosen mode; both go with every setting above.  A
        'static' or 'none' stage has no quantile to select, so the tail of its step is ONE elementwise launch at every image size
        (mi_sampler_step_direct_fwd): no cooperating workgroups, no status word.  With 'none' and a noise-predicting U-Net x0 grows without
        bound at the noisy end and the image saturates: the mode is meant for 'v' / 'x_start' models and deterministic solvers.

        For every keyword family: bad values, lengths and shapes raise ValueError before anything is launched (sample_call.parse), and a
        family that is left out is a ``StageCall`` field at its default -- such a call goes through exactly the workspaces, states, tables,
        graph keys and launches it went through before the family existed."""
        call = sample_call.parse(self, **{k: v for k, v in locals().items() if k != "self"})
        self._poll_status()                  # a cooperative launch of an EARLIER call gave up (its images are NaN): raise here, never silently
        self._status_stages = []
        call, lane, streams = self._place(call)
        # Packed-weight validation, once per call: identity up front, the content fingerprint launched and read AFTER the call's
        # work is enqueued.  A rare positive verdict (p.data updates behind the version counters: what was enqueued ran on stale packs) discards that
        # work and issues the SAME placed call again behind the whole check; injected noise (a stateful generator: no second run) keeps it all up front.
        img, done, stale = self._issue(call, lane, streams, full_check=call.noise.fn is not None)
        if stale:
            if streams is not None:
                torch.cuda.synchronize(img.device)
            self._status_stages = []
            img, done, _ = self._issue(call, lane, streams, full_check=True)
        return self._finish(call, lane, img, done)

    def _place(self, call: SampleCall):
        """-> (the call with its captions encoded and its tensors on the device, its lane, its stage streams or None off the GPU)"""
        self._reset_unets_all_one_device(device=call.device)
        text_embeds, text_masks, negative = call.text_embeds, call.text_masks, call.negative
        if call.texts is not None:
            text_embeds, text_masks = t5_encode_text(call.texts, name=self.text_encoder_name)
        if isinstance(negative, list):
            negative = t5_encode_text(negative, name=self.text_encoder_name)
        device = next(self.parameters()).device
        call = call.placed(device, text_embeds, text_masks, negative)
        # LANES: asynchronous calls alternate between SAMPLE_LANES independent sets of (stage streams, workspaces, graphs), so that two calls are in
        # flight side by side -- one call's kernels fill the launch floors and tails of the other's (42.8 K vs 37.7 K steps/s for the B = 32 cascade, DESIGN.md
        # section 6).  Calls on one lane stay ordered by its streams; lanes share only read-only state (weights, tables).  Synchronous calls use lane 0.
        lane, on_gpu = 0, L.backend() == "hip-gfx950"
        if call.is_async and on_gpu and SAMPLE_LANES > 1:
            lane = self._lane_rr = (getattr(self, "_lane_rr", -1) + 1) % SAMPLE_LANES
        return call, lane, self._call_streams(device, lane) if on_gpu else None

    def _call_streams(self, device, lane: int):
        """One HIP stream PER STAGE (graphs cannot be captured on the legacy default stream anyway).  Within a call stage s + 1 waits for stage s through an event;
        ACROSS calls the stages form a pipeline: with ``_async=True`` the caller's stream is never made to wait, so the (small, latency-bound) base stage of call k +
        1 runs on its stream while the super-resolution stage of call k still occupies the other -- each stage owns its workspace, so nothing is shared but the
        finished image handed down the cascade."""
        all_streams, lanes = getattr(self, "_stage_streams", None), max(1, SAMPLE_LANES)
        if all_streams is None or len(all_streams[0]) != len(self.unets) or all_streams[0][0].device != device or len(all_streams) != lanes:
            # earlier (smaller-image, latency-bound) stages get the higher stream priority: their short kernels then slot in between the
            # workgroups of the later stages' large ones instead of queueing behind them
            prio = int(os.environ.get("MINIMAGEN_STAGE_PRIORITY", "1"))
            if all_streams is not None:
                torch.cuda.synchronize(device)       # (rare: lane count / device changed) work queued on the old lanes' streams still owns the workspaces
            # ONE set of stage streams per process and shape, shared by every Imagen instance.  HIP multiplexes its streams onto GPU_MAX_HW_QUEUES
            # (default 4) hardware queues and torch hands out pool streams round robin: a second Imagen in the same process got streams whose hardware queue
            # was shared with the stream feeding them, and every node of a graph launched there paid ~16 us (a 150 ms sample() took 261 ms;
            # tools/gpu_realloc_slowdown.py, profiles/r04_second_instance_slowdown.txt).  The first set a process creates has never shown the sharing.
            key = (str(device), lanes, len(self.unets), prio)
            if key not in _STAGE_STREAMS:
                _STAGE_STREAMS[key] = [[torch.cuda.Stream(device=device, priority=(-1 if (prio and k + 1 < len(self.unets)) else 0))
                                        for k in range(len(self.unets))] for _ in range(lanes)]
            self._stage_streams = all_streams = _STAGE_STREAMS[key]
        self._stream = all_streams[0][-1]            # (benchmarks time the last stage's captured graph on its own stream)
        return all_streams[lane]

    def _issue(self, call: SampleCall, lane: int, streams, full_check: bool):
        """Enqueue the placed call: every stage on its own stream -> (the last stage's image, its completion event or None, whether the deferred
        weight check found the packs stale -- ``full_check``: the whole check up front instead)."""
        for unet in self.unets:
            unet.engine().pack() if full_check else unet.engine().pack_identity()
        on_gpu, B, noise = streams is not None, call.batch, call.noise
        on_stream = (lambda stage: torch.cuda.stream(streams[stage])) if on_gpu else null_context
        if on_gpu:
            inputs_ready = torch.cuda.current_stream(call.text_embeds.device).record_event()
        keeps = {kind: torch.cat((torch.ones(B, dtype=torch.bool), torch.zeros(0 if kind == 'plain' else B, dtype=torch.bool))) for kind in ('plain', 'scalar', 'table')}
        negative = call.negative or (None, None)
        lane_opts = dict(precision=call.precision, lane=lane, pipelined=bool(call.is_async and on_gpu and SAMPLE_LANES > 1))
        t_low = int(self.lowres_noise_schedule.num_timesteps * call.lowres_noise_level)
        # ---- pass 1, every stage on its own stream: what depends on the CAPTIONS only (text conditioning, the folded context rows, x_T, the
        # step tables) -- issued for all stages up front, so a later stage has it behind it when its low-resolution input arrives
        wss, begun = {}, {}
        for sc in call.stages:
            stage, unet, size, eng = sc.stage, self.unets[sc.stage], self.image_sizes[sc.stage], self.unets[sc.stage].engine()
            if on_gpu:
                streams[stage].wait_event(inputs_ready)
                # the stage streams read the caller's tensors after sample() has returned (_async) / after the caller may have dropped them: tell the
                # caching allocator, or a block freed on the caller's stream could be handed out again while a stage's text_cond launch is still queued
                for t_in in call.tensors:
                    if t_in.is_cuda:
                        t_in.record_stream(streams[stage])
            with on_stream(stage):
                wss[stage] = {}
                for kind in sc.kinds:                # every workspace the stage visits: its text, once per call
                    # per call, never sticky engine state: a later Unet.forward stays on the engine's default precision.  Guidance rescale and a run whose scales come
                    # from a table read both halves of the prediction: a workspace that never folds the guidance into the U-Net's tail; a plain run takes no negatives
                    ws = wss[stage][kind] = eng.workspace(B, keeps[kind].numel(), size, size, fold=not (kind == 'table' or (sc.rescale and kind == 'scalar')), **lane_opts)
                    eng.set_text(ws, call.text_embeds, call.text_masks, keeps[kind], *((None, None) if kind == 'plain' else negative))
                    if unet.lowres_cond:             # the augmentation level's timestep feeds the step tables (diffusion_model.py:68-69)
                        ws.lowres_times.fill_(t_low)
                if noise.fn is None:
                    begun[stage] = self._stage_begin(unet, (B, self.channels, size, size), wss[stage][sc.kinds[0]], sc, noise_scheduler=self.noise_schedulers[stage], noise=noise)
        # ---- pass 2: the cascade
        img, prev_done = call.start_image, None
        for sc in call.stages:
            stage, unet, size = sc.stage, self.unets[sc.stage], self.image_sizes[sc.stage]
            if on_gpu and prev_done is not None:
                streams[stage].wait_event(prev_done)
            with on_stream(stage):
                ws, shape = wss[stage][sc.kinds[0]], (B, self.channels, size, size)
                if unet.lowres_cond:
                    if on_gpu:
                        img.record_stream(streams[stage])
                    self._lowres_conditioning(unet, img, size, ws, call.lowres_noise_level, *noise, stage)
                    for other in wss[stage].values():           # drawn once, then copied
                        if other is not ws:
                            other.lowres.copy_(ws.lowres)
                            unet.engine().prepare_lowres(other)
                loop = dict(noise_scheduler=self.noise_schedulers[stage], noise=noise, use_graph=call.use_graph)
                if len(sc.runs) == 1 and sc.runs[0][0] != 'table':
                    img = self._p_sample_loop(unet, shape, ws, sc, begun=begun.get(stage), **loop)
                else:
                    img = S.run_plan(self, unet, shape, wss[stage], sc, begun.get(stage), max_states=MAX_SOLVER_STATES, **loop)
                if on_gpu:
                    prev_done = streams[stage].record_event()
        tokens = [] if full_check else [(unet.engine(), unet.engine().pack_begin()) for unet in self.unets]
        return img, prev_done, any(eng.pack_changed(tok) for eng, tok in tokens)

    def _finish(self, call: SampleCall, lane: int, img, done):
        """Status words, the asynchronous return, PIL images.  ``done``: the last stage's completion event (None off the GPU)."""
        if self._status_stages:
            self._status_pending.append((done, self._status_stages))
            self._status_stages = []
        if done is not None:
            if STRICT_STATUS and not call.is_async:
                done.synchronize()
                self._poll_status()
            if call.is_async:
                # pipelined use: the result is ready when ``done`` is (the caller waits on it before touching the images) -- per CALL: a later call on the OTHER
                # lane does not wait for it; capture it right after the call that produced the tensor (it travels on the tensor too), or use wait_pending_samples()
                self.last_sample_done = self._lane_done[lane] = done
                if not call.return_pil:
                    img.sample_done = done
                    return img
            caller_stream = torch.cuda.current_stream(img.device)
            caller_stream.wait_event(done)                   # (_async with PIL images: the device -> host copy below runs on the caller's stream)
            img.record_stream(caller_stream)
        if not call.return_pil:
            return img
        pil = _to_pil_images(img)
        self.check_device_status()
        return pil

    def _poll_status(self, block: bool = False):
        """Status of the kernels whose workgroups wait for each other (the grouped sampler tail).  Such a launch is fail-stop: when a wait
        runs out it sets a sticky error word and turns the image -- and everything sampled from it afterwards -- into NaN.  Every sample()
        call copies the word to pinned host memory behind its last launch; this looks at the calls whose completion event has fired
        (``block=True``: waits for all of them) and raises MinImagenHipError for a failed one.  Called at every sample() entry, by
        wait_pending_samples() and check_device_status().  Recovery is automatic: the stage state re-zeroes its sync buffer before its next
        launch and keeps the separate (non-cooperative) kernels from then on."""
        failed, rest = [], []
        for done, stages in self._status_pending:
            if done is not None:
                if block:
                    done.synchronize()
                elif not done.query():
                    rest.append((done, stages))
                    continue
            for st, stage, shape in stages:
                err = int(st.group_err_host.item())
                if err and not st.group_failed:
                    st.group_failed, st.group_heal = True, True
                    failed.append(f"stage {stage} {shape}: {err:#x}")
                elif err:
                    failed.append(f"stage {stage} {shape}: {err:#x} (call queued behind the failed one)")
        self._status_pending = rest
        if failed:
            raise L.MinImagenHipError("grouped sampler tail: a workgroup timed out waiting for its image's other workgroups (" + "; ".join(failed) +
                                      "); the images of that sample() call are NaN.  The stage falls back to the separate kernels from the next call on.")

    def check_device_status(self):
        """Host-side check (waits for every sample() call in flight): no kernel whose workgroups wait for each other gave up waiting."""
        self._poll_status(block=True)

    def wait_pending_samples(self, stream=None):
        """Make ``stream`` (default: the caller's current stream) wait for the latest ``sample(_async=True)`` call of EVERY call lane; raises
        if a call that has already completed reported a failed cooperative launch (check_device_status() waits on the host and covers all)."""
        for ev in self._lane_done.values():
            (stream if stream is not None else torch.cuda.current_stream()).wait_event(ev)
        self._poll_status()


def _to_pil_images(img: torch.Tensor):
    """torchvision.transforms.ToPILImage on a float CHW tensor (Imagen.py:508): mul(255) then truncate to uint8."""
    import numpy as np
    from PIL import Image
    arr = img.detach().to('cpu').mul(255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().numpy()
    return [Image.fromarray(np.ascontiguousarray(a)) for a in arr]
