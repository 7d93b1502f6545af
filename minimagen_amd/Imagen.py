"""``Imagen`` with the reference's constructor and ``sample`` API (minimagen/Imagen.py), whose cascaded
reverse-diffusion loop runs as HIP kernels replayed from a HIP graph on MI355X."""
from __future__ import annotations

import os
from typing import Callable, List, Literal, Tuple, Union

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib as L
from . import sampler as S
from . import train_ops
from .Unet import Unet
from .diffusion_model import GaussianDiffusion
from .helpers import (cast_tuple, default, eval_decorator, exists, module_device, normalize_neg_one_to_one, resize_image_to)
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
_STAGE_STREAMS = {}          # (device, lanes, stages, priority mode) -> [lane][stage] HIP streams, process-wide (see sample())


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
            vals = tuple(val) if isinstance(val, (list, tuple)) else (val,) * num_unets      # (the parameter JSON turns tuples into lists)
            if len(vals) != num_unets:
                raise ValueError(f"{name} needs one value per U-Net ({num_unets}), got {len(vals)}")
            for v in vals:
                if not ok(v):
                    raise ValueError(f"{name} must be {what}, got {v!r}")
            return vals
        self.pred_objectives = per_unet(pred_objectives, "pred_objectives", lambda v: isinstance(v, str) and v in GaussianDiffusion.OBJECTIVES,
                                        f"one of {GaussianDiffusion.OBJECTIVES}")
        self.min_snr_loss_weight = per_unet(min_snr_loss_weight, "min_snr_loss_weight", lambda v: isinstance(v, bool), "a bool")
        self.min_snr_gamma = tuple(float(v) for v in per_unet(
            min_snr_gamma, "min_snr_gamma", lambda v: not isinstance(v, bool) and isinstance(v, (int, float)) and v > 0. and v == v, "a positive number"))
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

    # ------------------------------------------------------------------ sampling
    # ------------------------------------------------------------------ sampling (the loop itself: minimagen_amd/sampler.py)
    def _stage_state(self, ws, sched: GaussianDiffusion, B: int, n: int, solver=None, eng=None):
        return S.stage_state(ws, sched, B, n, solver, eng, MAX_SOLVER_STATES)

    def _stage_begin(self, unet: Unet, shape, **kw):          # -> (stage state, injected noise)
        return S.stage_begin(unet, shape, max_states=MAX_SOLVER_STATES, **kw)

    def _p_sample_loop(self, unet: Unet, shape, **kw):        # Imagen.py:373-420 -> the stage's image
        return S.p_sample_loop(self, unet, shape, group_max=SAMPLER_GROUP_MAX if SAMPLER_GROUP else 0, max_states=MAX_SOLVER_STATES, **kw)

    def _parse_solver(self, sample_steps, sampler, sampler_eta):
        """Per stage: None (the reference's loop on all T timesteps) or (S, sampler, eta).  Host only; raises ValueError on bad values."""
        n_stages = len(self.unets)
        if sampler is not None and sampler not in GaussianDiffusion.SAMPLERS:
            raise ValueError(f"sampler must be one of {GaussianDiffusion.SAMPLERS}, got {sampler!r}")
        name = default(sampler, 'ddpm')
        if sampler_eta is not None:
            if name != 'ddim':
                raise ValueError("sampler_eta goes with sampler='ddim' only")
            if isinstance(sampler_eta, bool) or not isinstance(sampler_eta, (int, float)) or not 0. <= float(sampler_eta) <= 1.:
                raise ValueError(f"sampler_eta must be a number in [0, 1], got {sampler_eta!r}")
        eta = {'ddpm': 1., 'ddim': float(default(sampler_eta, 0.)), 'dpmpp_2m': 0.}[name]
        if isinstance(sample_steps, (list, tuple)):
            steps = tuple(sample_steps)
            if len(steps) != n_stages:
                raise ValueError(f"sample_steps needs one value per stage ({n_stages}), got {len(steps)}")
        else:
            steps = (sample_steps,) * n_stages
        out = []
        for S, sched in zip(steps, self.noise_schedulers):
            T = sched.num_timesteps
            if S is None:
                S = T
            if isinstance(S, bool) or not isinstance(S, int) or not 2 <= S <= T:
                raise ValueError(f"sample_steps must be an int in [2, {T}] for a stage trained with {T} timesteps, got {S!r}")
            out.append(None if (S == T and name == 'ddpm') else (S, name, eta))
        return out

    def _parse_inpaint(self, batch_size: int, inpaint_images, inpaint_masks, start_image, start_at_stage, stop_at_stage):
        """-> (first stage, one past the last stage, (images float32 [B, C, H, W], masks uint8 [B, Hm, Wm]) or None, start image float32 or None),
        the tensors still where the caller has them.  Host only; raises ValueError on bad or inconsistent values."""
        n_stages = len(self.unets)

        def stage_index(v, name, lo, hi):
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
                raise ValueError(f"{name} must be an int in [{lo}, {hi}] for a cascade of {n_stages} stages, got {v!r}")
            return v

        def images(t, name):
            if not torch.is_tensor(t) or t.dim() != 4 or not t.is_floating_point():
                raise ValueError(f"{name} must be a float tensor [B, {self.channels}, H, W]")
            if t.shape[0] != batch_size:
                raise ValueError(f"{name}: batch {t.shape[0]} does not match the text batch {batch_size}")
            if t.shape[1] != self.channels:
                raise ValueError(f"{name}: {t.shape[1]} channels, the model has {self.channels}")
            if t.shape[2] != t.shape[3] or t.shape[2] < 1:
                raise ValueError(f"{name} must be square, got {tuple(t.shape[2:])}")
            return t.detach().to(torch.float32)

        stop = n_stages if stop_at_stage is None else stage_index(stop_at_stage, "stop_at_stage", 1, n_stages)
        start = 0
        if (start_image is None) != (start_at_stage is None):
            raise ValueError("start_image and start_at_stage go together")
        if start_at_stage is not None:
            start = stage_index(start_at_stage, "start_at_stage", 1, n_stages - 1)
            if start >= stop:
                raise ValueError(f"start_at_stage = {start} must be below stop_at_stage = {stop}")
            if not self.unets[start].lowres_cond:
                raise ValueError(f"stage {start} takes no low-resolution conditioning image: it cannot start from one")
            start_image = images(start_image, "start_image")
        inpaint = None
        if (inpaint_images is None) != (inpaint_masks is None):
            raise ValueError("inpaint_images and inpaint_masks go together")
        if inpaint_images is not None:
            inpaint_images = images(inpaint_images, "inpaint_images")
            m = inpaint_masks
            if not torch.is_tensor(m) or m.dim() not in (3, 4) or (m.dim() == 4 and m.shape[1] != 1):
                raise ValueError("inpaint_masks must be a tensor [B, H, W] or [B, 1, H, W]")
            if m.shape[0] != batch_size:
                raise ValueError(f"inpaint_masks: batch {m.shape[0]} does not match the text batch {batch_size}")
            m = m.detach().reshape(m.shape[0], m.shape[-2], m.shape[-1])
            if m.shape[1] < 1 or m.shape[2] < 1:
                raise ValueError("inpaint_masks: empty")
            if m.dtype != torch.bool and not bool(((m == 0) | (m == 1)).all()):
                raise ValueError("inpaint_masks must hold 0 / 1 (or be bool)")
            inpaint = (inpaint_images, m.to(torch.uint8))
        return start, stop, inpaint, start_image

    def _parse_init(self, batch_size: int, init_images, init_strength, solvers, first_stage: int, end_stage: int):
        """-> (init images float32 [B, C, H, W] still where the caller has them, or None; per stage None -- the stage starts from pure noise -- or
        a0, the number of loop steps it skips: sampler.init_start_step).  A strength for a stage the call does not run is ignored.  Host only;
        raises ValueError on bad or inconsistent values."""
        n_stages = len(self.unets)
        if init_images is None and init_strength is None:
            return None, [None] * n_stages
        if init_images is None or init_strength is None:
            raise ValueError("init_images and init_strength go together")
        t = init_images
        if not torch.is_tensor(t) or t.dim() != 4 or not t.is_floating_point():
            raise ValueError(f"init_images must be a float tensor [B, {self.channels}, H, W]")
        if t.shape[0] != batch_size:
            raise ValueError(f"init_images: batch {t.shape[0]} does not match the text batch {batch_size}")
        if t.shape[1] != self.channels:
            raise ValueError(f"init_images: {t.shape[1]} channels, the model has {self.channels}")
        if t.shape[2] != t.shape[3] or t.shape[2] < 1:
            raise ValueError(f"init_images must be square, got {tuple(t.shape[2:])}")
        if isinstance(init_strength, (list, tuple)):
            strengths = list(init_strength)
            if len(strengths) != n_stages:
                raise ValueError(f"init_strength needs one entry per stage ({n_stages}), got {len(strengths)}")
        else:
            if init_strength is None or isinstance(init_strength, bool) or not isinstance(init_strength, (int, float)):
                raise ValueError(f"init_strength must be a number in (0, 1] or a list with a number or None per stage, got {init_strength!r}")
            strengths = [init_strength] * n_stages
        starts = [None] * n_stages
        for stage, v in enumerate(strengths):
            if v is None:
                continue
            n_steps = self.noise_schedulers[stage].num_timesteps if solvers[stage] is None else solvers[stage][0]
            a0 = S.init_start_step(n_steps, v)                   # (validates the value of every entry, run or not)
            if first_stage <= stage < end_stage:
                starts[stage] = a0
        if all(a0 is None for a0 in starts):
            raise ValueError("init_strength: every stage the call runs has None")
        return t.detach().to(torch.float32), starts

    def _parse_guidance(self, batch_size: int, cond_scale, texts, text_embeds, text_masks, negative_texts, negative_text_embeds,
                        negative_text_masks, guidance_rescale, guided: bool = None):
        """``guided``: whether any step of the call is guided (None: ``cond_scale`` != 1, a call without a guidance schedule).
        -> (phi: 0. when off, negative captions: None, a list of ``batch_size`` strings, or (embeds, mask or None) still where the caller has
        them).  Host only; raises ValueError on bad or inconsistent values."""
        phi = 0.
        if guidance_rescale is not None:
            if isinstance(guidance_rescale, bool) or not isinstance(guidance_rescale, (int, float)) or not 0. <= float(guidance_rescale) <= 1.:
                raise ValueError(f"guidance_rescale must be a number in [0, 1], got {guidance_rescale!r}")
            phi = float(guidance_rescale)
        negative = None
        if negative_texts is not None and negative_text_embeds is not None:
            raise ValueError("pass negative_texts or negative_text_embeds, not both")
        if negative_text_masks is not None and negative_text_embeds is None:
            raise ValueError("negative_text_masks goes with negative_text_embeds")
        masked = exists(text_masks) or not exists(text_embeds)              # (captions encoded here always come with masks)
        if negative_texts is not None:
            if isinstance(negative_texts, str):
                negative_texts = [negative_texts] * batch_size
            if not isinstance(negative_texts, (list, tuple)) or not all(isinstance(t, str) for t in negative_texts):
                raise ValueError("negative_texts must be a string or a list of strings")
            if len(negative_texts) != batch_size:
                raise ValueError(f"negative_texts: batch {len(negative_texts)} does not match the text batch {batch_size}")
            if not masked:
                raise ValueError("negative_texts are encoded with masks: pass text_masks with text_embeds (the captions and the negative captions "
                                 "must both carry masks, or neither)")
            negative = list(negative_texts)
        elif negative_text_embeds is not None:
            e, m = negative_text_embeds, negative_text_masks
            if not torch.is_tensor(e) or e.dim() != 3 or not e.is_floating_point():
                raise ValueError("negative_text_embeds must be a float tensor [B, L, E]")
            if e.shape[0] != batch_size:
                raise ValueError(f"negative_text_embeds: batch {e.shape[0]} does not match the text batch {batch_size}")
            if e.shape[2] != self.text_embed_dim:
                raise ValueError(f"negative_text_embeds: embedding dimension {e.shape[2]}, the model has {self.text_embed_dim}")
            if m is not None and (not torch.is_tensor(m) or tuple(m.shape) != tuple(e.shape[:2])):
                raise ValueError(f"negative_text_masks must be a tensor {tuple(e.shape[:2])} like negative_text_embeds")
            if masked != (m is not None):
                raise ValueError("negative prompts: the captions and the negative captions must both carry masks, or neither")
            if m is None and exists(text_embeds) and text_embeds.shape[1] != e.shape[1]:
                raise ValueError(f"negative prompts: unmasked captions of different lengths ({text_embeds.shape[1]} and {e.shape[1]}) cannot be "
                                 "joined; pass masks")
            negative = (e.detach(), None if m is None else m.detach())
        if (phi or negative is not None) and not (cond_scale != 1. if guided is None else guided):
            raise ValueError("negative prompts and guidance_rescale need cond_scale != 1 (or a guidance schedule with a guided step): at 1 the second "
                             "half of the guidance batch is never evaluated")
        return phi, negative

    def _parse_guidance_schedule(self, batch_size: int, cond_scale, solvers, guidance_interval, guidance_schedule):
        """-> None when neither keyword is given, else per stage None (``cond_scale`` on every step, the call as it was) or that stage's guidance
        scales, float64 [S] or [S, B] in execution order (sampler.guidance_scale_table).  Host only; raises ValueError on bad values."""
        if guidance_interval is None and guidance_schedule is None:
            return None
        n_stages = len(self.unets)

        def per_stage(v, name, single):
            if single(v):
                return [v] * n_stages
            if not isinstance(v, (list, tuple)) or len(v) != n_stages:
                raise ValueError(f"{name} needs one entry per stage ({n_stages})")
            return list(v)

        def number(v):
            return not isinstance(v, bool) and isinstance(v, (int, float))

        intervals = [None] * n_stages
        if guidance_interval is not None:
            is_pair = lambda v: isinstance(v, (list, tuple)) and len(v) == 2 and all(number(x) for x in v)
            intervals = per_stage(guidance_interval, "guidance_interval", is_pair)
            for iv in intervals:
                if iv is None:
                    continue
                if not is_pair(iv) or not 0. <= float(iv[0]) <= float(iv[1]) <= 1.:
                    raise ValueError(f"guidance_interval must be (lo, hi) with 0 <= lo <= hi <= 1 (or None for a stage), got {iv!r}")
            if all(iv is None for iv in intervals):
                raise ValueError("guidance_interval: every stage's entry is None")
            intervals = [None if iv is None else (float(iv[0]), float(iv[1])) for iv in intervals]
        schedules = [None] * n_stages
        if guidance_schedule is not None:
            if cond_scale != 1.:
                raise ValueError("guidance_schedule is the scale itself: leave cond_scale at 1")
            schedules = per_stage(guidance_schedule, "guidance_schedule", callable)
            if all(s is None for s in schedules):
                raise ValueError("guidance_schedule: every stage's entry is None")
        elif cond_scale == 1.:
            raise ValueError("guidance_interval needs cond_scale != 1 (or a guidance_schedule): outside the interval the scale is 1 already")
        if isinstance(cond_scale, bool) or not isinstance(cond_scale, (int, float)) or cond_scale != cond_scale or abs(cond_scale) == float("inf"):
            raise ValueError(f"cond_scale must be a finite number, got {cond_scale!r}")
        tables = []
        for stage, sched in enumerate(self.noise_schedulers):
            if intervals[stage] is None and schedules[stage] is None:
                tables.append(None)
                continue
            T = sched.num_timesteps
            tau = torch.arange(T) if solvers[stage] is None else sched.sampling_timestep_map(solvers[stage][0])
            tables.append(S.guidance_scale_table(tau, T, batch_size, cond_scale, intervals[stage], schedules[stage]))
        return tables

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
               _use_graph: bool = True, _precision: str = None, _async: bool = False, _revalidated: bool = False,
               sample_steps: Union[int, List[int], Tuple[int, ...]] = None, sampler: str = None, sampler_eta: float = None,
               inpaint_images: torch.Tensor = None, inpaint_masks: torch.Tensor = None, start_image: torch.Tensor = None,
               start_at_stage: int = None, stop_at_stage: int = None,
               negative_texts: Union[str, List[str]] = None, negative_text_embeds: torch.Tensor = None, negative_text_masks: torch.Tensor = None,
               guidance_rescale: float = None, guidance_interval=None, guidance_schedule=None,
               init_images: torch.Tensor = None, init_strength=None):
        """minimagen/Imagen.py:424-510.  Private keyword-only extras (not in the reference): ``_noise(shape)`` injects a
        host noise stream in the reference's draw order (parity runs); otherwise noise is Philox keyed by
        (``_seed``, ``_sample_offset`` + row, stage, step, element) so a sharded batch reproduces the unsharded one;
        ``_precision`` = "fp32" (default) or "half" (single-fp16-term matrix-core contractions, see engine.UnetEngine.precision);
        ``_async=True`` returns without making the caller's stream wait (``self.last_sample_done`` / the returned tensor's ``sample_done`` is THIS call's completion event; ``wait_pending_samples()`` covers every lane): successive
        calls then pipeline across the per-stage streams (the base stage of the next batch under the super-resolution stage of this one).

        Sampling in fewer steps (keyword-only, not in the reference): ``sample_steps`` = S, an int or one int per stage, 2 <= S <= T of
        that stage's schedule (None: T) walks S of the trained timesteps, tau_k = round(k (T-1) / (S-1)), one U-Net evaluation each.
        ``sampler`` = 'ddpm' (default: the reference's ancestral step on the subsequence), 'ddim' (eta = ``sampler_eta``, default 0) or
        'dpmpp_2m' (DPM-Solver++ 2M on the thresholded x0, deterministic); ``sampler_eta`` in [0, 1] goes with 'ddim' only.  A call with
        none of them, or with S = T and 'ddpm', IS the reference's loop (same tables, graphs and kernels as before these arguments
        existed).  Tables: GaussianDiffusion.sampler_tables.  Bad values raise ValueError before anything is launched.

        Conditioning on pixels the caller has (keyword-only, not in the reference).  ``inpaint_images`` ([B, C, H, W]
        float in [0, 1], square, any size) with ``inpaint_masks`` ([B, H, W] or [B, 1, H, W], bool or 0/1, nonzero = "known, keep"): every
        stage re-imposes the known pixels -- the images resized to its size (cubic, antialiased when shrinking), the masks by nearest
        neighbour -- at the noise level of EVERY step, inside the sampler tails, for every ``sampler`` / ``sample_steps``; the returned
        images carry them.  One pass per step: no RePaint resampling.  ``start_image`` ([B, C, H, W] in [0, 1], square, any size) with
        ``start_at_stage`` = s >= 1 skips the stages below s and stands in for the output of stage s - 1 (run only the super-resolution
        stage on an image of the caller's); ``stop_at_stage`` = s runs the stages below s and returns that stage's image.  The noise is
        keyed by the stage INDEX, so a cascade cut in two this way gives the bits of the whole.  A call with none of these goes through
        exactly the states, tables, graphs and kernels it went through before they existed.

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
        (whatever its objective), before x0 and the dynamic threshold.  Both go with every setting above.  Bad values raise ValueError
        before anything is launched; a call with neither goes through exactly the workspaces, states, graphs and kernels it went through
        before they existed.  Nothing here has been tried on a trained model: what is checked is the arithmetic.

        Guidance over the steps (keyword-only, not in the reference).  ``guidance_interval`` = (lo, hi), 0 <= lo <= hi <= 1,
        one pair for every stage or a list with a pair or None per stage (needs ``cond_scale`` != 1 or a schedule): the step at trained
        timestep tau is guided with ``cond_scale`` iff lo (T - 1) <= tau <= hi (T - 1) (Kynkaanniemi et al. 2024); every other step runs
        unguided, over B rows of the U-Net instead of 2 B.  ``guidance_schedule`` IS the scale per step (``cond_scale`` stays 1): a callable
        f(u) -> float of u = tau / (T - 1) for every stage, or a list with one entry per stage -- None, a callable, or a float tensor /
        sequence [S] or [S, B] (per row), entry 0 the first step executed (the noisiest).  With both, steps outside the interval get scale 1.
        A step whose scales are all exactly 1 is unguided (negative prompts and ``guidance_rescale``, the identity there, are skipped; they
        need one guided step somewhere).  A stage moves between its B-row and its 2 B-row workspace at the run boundaries (x, the
        dpmpp_2m history and the step index are handed over; same noise stream); an interval of (0, 1), a constant schedule s or an
        all-ones schedule IS the call with ``cond_scale`` = s / 1.  Bad values, lengths and shapes raise ValueError before anything is launched.

        Starting from an image (SDEdit / "img2img"; keyword-only, not in the reference).  ``init_images`` ([B, C, H, W]
        float in [0, 1], square, any size; resized per stage like ``inpaint_images``) with ``init_strength`` = s in (0, 1] for every stage, or
        a list with s or None (that stage starts from pure noise, as without the keywords) per stage: a stage of S loop steps skips its
        first a0 = S - m, m = min(S, max(1, floor(s S + 0.5))) (sampler.init_start_step), and runs the other m from
        x = sqrt(abar_tau) y' + sqrt(1 - abar_tau) eps at tau = the trained timestep of step a0 (GaussianDiffusion.init_start_coefs) -- eps IS
        the stage's own x_T draw and every other draw keeps its index in the full loop, so a sharded batch reproduces the unsharded one and
        ``_noise`` is called in the order it is called today.  With every ``sampler`` / ``sample_steps`` ('dpmpp_2m': the first executed
        step is first order), with inpainting (blend 0 at the starting level), with ``start_image`` / ``start_at_stage`` / ``stop_at_stage`` (a
        strength for a stage that does not run is ignored) and with the guidance keywords, whose intervals and schedules stay indexed by the
        step of the FULL loop ([S] / [S, B] keep their shape, entry a0 is the first one executed; "one guided step somewhere" means an
        executed one).  One strength per stage, not per row; no RePaint resampling.  Bad values raise ValueError before anything is
        launched; a call without the two goes through exactly the workspaces, states, tables, graph keys and launches it goes through today.
        Nothing here has been tried on a trained model: what is checked is the arithmetic."""
        solvers = self._parse_solver(sample_steps, sampler, sampler_eta)
        rescale, negative, scale_tabs = 0., None, None
        if exists(text_embeds) or exists(texts):
            n_rows = text_embeds.shape[0] if exists(text_embeds) else len(texts)
            first_stage, end_stage, inpaint, start_image = self._parse_inpaint(n_rows, inpaint_images, inpaint_masks, start_image, start_at_stage, stop_at_stage)
            init_images, init_starts = self._parse_init(n_rows, init_images, init_strength, solvers, first_stage, end_stage)
            scale_tabs = self._parse_guidance_schedule(n_rows, cond_scale, solvers, guidance_interval, guidance_schedule)
            guided = None
            if scale_tabs is not None:                           # (of the steps a stage executes: a loop that starts at an init image skips its first ones)
                guided = any(cond_scale != 1. if scale_tabs[s] is None else bool((scale_tabs[s][init_starts[s] or 0:] != 1.).any())
                             for s in range(first_stage, end_stage))
            rescale, negative = self._parse_guidance(n_rows, cond_scale, texts, text_embeds, text_masks,
                                                     negative_texts, negative_text_embeds, negative_text_masks, guidance_rescale, guided)
        call_args = dict(guidance_interval=guidance_interval, guidance_schedule=guidance_schedule, negative_texts=negative_texts, negative_text_embeds=negative_text_embeds, negative_text_masks=negative_text_masks,
                         guidance_rescale=guidance_rescale, init_images=init_images, init_strength=init_strength, inpaint_images=inpaint_images, inpaint_masks=inpaint_masks, start_image=start_image, start_at_stage=start_at_stage,
                         stop_at_stage=stop_at_stage, sample_steps=sample_steps, sampler=sampler, sampler_eta=sampler_eta, texts=texts, text_masks=text_masks, text_embeds=text_embeds, cond_scale=cond_scale, lowres_sample_noise_level=lowres_sample_noise_level,
                         return_pil_images=return_pil_images, device=device, _noise=_noise, _seed=_seed, _sample_offset=_sample_offset,
                         _use_graph=_use_graph, _precision=_precision, _async=_async)
        device = default(device, self.device)
        self._poll_status()                  # a cooperative launch of an EARLIER call gave up (its images are NaN): raise here, never silently
        self._status_stages = []
        self._reset_unets_all_one_device(device=device)
        if exists(texts) and not exists(text_embeds):
            text_embeds, text_masks = t5_encode_text(texts, name=self.text_encoder_name)
            text_embeds, text_masks = map(lambda t: t.to(device), (text_embeds, text_masks))
        assert exists(text_embeds), 'text or text encodings must be passed into Imagen'
        if isinstance(negative, list):
            negative = t5_encode_text(negative, name=self.text_encoder_name)
        assert not (exists(text_embeds) and text_embeds.shape[-1] != self.text_embed_dim), \
            f'invalid text embedding dimension being passed in (should be {self.text_embed_dim})'
        # the runs of every stage's guidance plan, (kind, first step, one past the last, scale): ONE run over all steps for a call without
        # a schedule or interval -- and for a table that is one row-uniform value on every step, which IS that call (sampler.guidance_plan)
        plans = {}
        for stage in range(first_stage, end_stage):
            w_stage = None if scale_tabs is None else scale_tabs[stage]
            n_steps = self.noise_schedulers[stage].num_timesteps if solvers[stage] is None else solvers[stage][0]
            a0 = init_starts[stage] or 0                         # a stage that starts from an init image: the plan of the steps [a0, S) it executes
            plans[stage] = [('plain' if cond_scale == 1. else 'scalar', a0, n_steps, cond_scale)] if w_stage is None else \
                [(kind, a + a0, b + a0, scale) for kind, a, b, scale in S.guidance_plan(w_stage[a0:])]
        any_guided = any(kind != 'plain' for runs in plans.values() for kind, *_ in runs)
        assert not (any_guided and not self.can_classifier_guidance), \
            'imagen was not trained with conditional dropout, and thus one cannot use classifier free guidance (cond_scale anything other than 1)'
        batch_size = text_embeds.shape[0]
        device = next(self.parameters()).device
        lowres_sample_noise_level = default(lowres_sample_noise_level, self.lowres_sample_noise_level)
        keeps = {kind: torch.cat((torch.ones(batch_size, dtype=torch.bool), torch.zeros(0 if kind == 'plain' else batch_size, dtype=torch.bool)))
                 for kind in ('plain', 'scalar', 'table')}
        text_embeds = text_embeds.to(device)
        text_masks = text_masks.to(device) if exists(text_masks) else None
        if inpaint is not None:
            inpaint = tuple(t.to(device).contiguous() for t in inpaint) + (self.auto_normalize_img,)
        if start_image is not None:
            start_image = start_image.to(device).contiguous()
        if init_images is not None:
            init_images = init_images.to(device).contiguous()
        pixel_inputs = [t for t in (inpaint or ())[:2] + (start_image, init_images) if t is not None]
        if negative is not None:            # read by the stage streams like the captions (record_stream below)
            negative = tuple(None if t is None else t.to(device) for t in negative)
            pixel_inputs += [t for t in negative if t is not None]
        neg_text = {} if negative is None else dict(negative_embeds=negative[0], negative_mask=negative[1])

        # One HIP stream PER STAGE (graphs cannot be captured on the legacy default stream anyway).  Within a call stage s + 1 waits for
        # stage s through an event; ACROSS calls the stages form a pipeline: with ``_async=True`` the caller's stream is never made to
        # wait, so the (small, latency-bound) base stage of call k + 1 runs on its stream while the super-resolution stage of call k
        # still occupies the other -- each stage owns its workspace, so nothing is shared but the finished image handed down the cascade.
        on_gpu = L.backend() == "hip-gfx950"
        # Packed-weight validation, once per call.  Identity (pointers, version counters: host only) up front; the content fingerprint -- device
        # work on the caller's stream + one small device -> host copy -- is launched and read AFTER this call's work is enqueued (see
        # engine.pack_identity).  A rare positive verdict discards the enqueued work and runs the call again on fresh packs.  Injected noise
        # (a stateful host generator: the call cannot be repeated) keeps the whole check up front.
        for unet in self.unets:
            if _noise is not None or _revalidated:
                unet.engine().pack()
            else:
                unet.engine().pack_identity()
        # LANES: asynchronous calls alternate between SAMPLE_LANES independent sets of (stage streams, workspaces, graphs), so that two
        # calls are in flight side by side -- the kernels of one call's stages fill the launch floors and tails of the other's (measured:
        # 42.8 K vs 37.7 K steps/s for the B = 32 cascade).  Calls on one lane stay ordered by its streams; lanes share
        # only read-only state (weights, tables).  Synchronous calls use lane 0.
        lane = 0
        if _async and on_gpu and SAMPLE_LANES > 1:
            lane = self._lane_rr = (getattr(self, "_lane_rr", -1) + 1) % SAMPLE_LANES
        if on_gpu:
            all_streams = getattr(self, "_stage_streams", None)
            if all_streams is None or len(all_streams[0]) != len(self.unets) or all_streams[0][0].device != device or len(all_streams) != max(1, SAMPLE_LANES):
                # earlier (smaller-image, latency-bound) stages get the higher stream priority: their short kernels then slot in between the
                # workgroups of the later stages' large ones instead of queueing behind them
                prio = int(os.environ.get("MINIMAGEN_STAGE_PRIORITY", "1"))
                if all_streams is not None:
                    torch.cuda.synchronize(device)       # (rare: lane count / device changed) work queued on the old lanes' streams still owns the workspaces
                # ONE set of stage streams per process and shape, shared by every Imagen instance.  HIP multiplexes its streams onto
                # GPU_MAX_HW_QUEUES (default 4) hardware queues, and torch hands out pool streams round robin: a second Imagen built in the
                # same process got streams whose hardware queue was shared with the stream feeding them, and every node of a graph launched
                # there paid ~16 us (2.7 ms per 170-node launch: a 150 ms sample() took 261 ms; tools/gpu_realloc_slowdown.py,
                # profiles/r04_second_instance_slowdown.txt -- the device buffers had nothing to do with it).  The first set a process creates
                # has never shown the sharing; keeping it for all instances makes the mapping a constant.
                key = (str(device), max(1, SAMPLE_LANES), len(self.unets), prio)
                all_streams = _STAGE_STREAMS.get(key)
                if all_streams is None:
                    all_streams = _STAGE_STREAMS[key] = [[torch.cuda.Stream(device=device, priority=(-1 if (prio and k + 1 < len(self.unets)) else 0))
                                                          for k in range(len(self.unets))] for _ in range(max(1, SAMPLE_LANES))]
                self._stage_streams = all_streams
            streams = all_streams[lane]
            self._stream = all_streams[0][-1]            # (benchmarks time the last stage's captured graph on its own stream)
            caller_stream = torch.cuda.current_stream(device)
            inputs_ready = caller_stream.record_event()
        from .helpers import null_context
        precision = _precision if _precision is not None else os.environ.get("MINIMAGEN_PRECISION", "fp32")
        stages = list(enumerate(zip(self.unets, self.sample_channels, self.image_sizes, self.noise_schedulers)))[first_stage:end_stage]
        known = {} if inpaint is None else dict(inpaint=inpaint)        # (a call without known pixels passes nothing new down)
        # ... and neither does a noise-predicting stage: only another objective names itself (it selects the stage's coefficient table)
        extras = {stage: dict(known, **({} if self.pred_objectives[stage] == 'noise' else dict(objective=self.pred_objectives[stage])),
                              **({} if init_starts[stage] is None else dict(init=(init_images, self.auto_normalize_img))))
                  for stage, _ in stages}
        starts = {stage: {} if init_starts[stage] is None else dict(start=init_starts[stage]) for stage, _ in stages}
        # guidance rescale reads both halves of the prediction: a workspace of its own that never folds the guidance into the U-Net's tail --
        # and so does a run whose scales come from a table; an unguided run (B rows) takes neither, nor the negative captions
        unfolded = {kind: dict(fold=False) if (kind == 'table' or (rescale and kind == 'scalar')) else {} for kind in keeps}
        rescaled = {kind: dict(rescale=rescale) if (rescale and kind != 'plain') else {} for kind in keeps}
        # ---- pass 1, every stage on its own stream: what depends on the CAPTIONS only (text conditioning, the folded context rows, x_T, the
        # step tables) -- issued for all stages up front, so a later stage has it behind it when its low-resolution input arrives
        wss, begun = {}, {}
        for stage, (unet, channel, image_size, noise_scheduler) in stages:
            if on_gpu:
                streams[stage].wait_event(inputs_ready)
                # the stage streams read the caller's tensors after sample() has returned (_async) / after the caller may have dropped
                # them: tell the caching allocator, or a block freed on the caller's stream could be handed out again while a stage's
                # text_cond launch is still queued
                for t_in in (text_embeds, text_masks, *pixel_inputs):
                    if t_in is not None and t_in.is_cuda:
                        t_in.record_stream(streams[stage])
            with (torch.cuda.stream(streams[stage]) if on_gpu else null_context()):
                eng = unet.engine()
                wss[stage] = {}
                for kind in dict.fromkeys(run[0] for run in plans[stage]):          # every workspace the stage visits: its text, once per call
                    # per call, never sticky engine state: a later Unet.forward stays on the engine's default precision
                    ws = wss[stage][kind] = eng.workspace(batch_size, keeps[kind].numel(), image_size, image_size, precision=precision, lane=lane,
                                                          pipelined=bool(_async and on_gpu and SAMPLE_LANES > 1), **unfolded[kind])
                    eng.set_text(ws, text_embeds, text_masks, keeps[kind], **({} if kind == 'plain' else neg_text))
                    if unet.lowres_cond:             # the augmentation level's timestep feeds the step tables (diffusion_model.py:68-69)
                        ws.lowres_times.fill_(int(self.lowres_noise_schedule.num_timesteps * lowres_sample_noise_level))
                if _noise is None:
                    begun[stage] = self._stage_begin(unet, (batch_size, self.channels, image_size, image_size), noise_scheduler=noise_scheduler,
                                                     ws=wss[stage][plans[stage][0][0]], seed=_seed, sample0=_sample_offset, stage=stage, solver=solvers[stage], **extras[stage], **starts[stage])
        # ---- pass 2: the cascade
        img, prev_done = start_image, None
        for stage, (unet, channel, image_size, noise_scheduler) in stages:
            if on_gpu and prev_done is not None:
                streams[stage].wait_event(prev_done)
            with (torch.cuda.stream(streams[stage]) if on_gpu else null_context()):
                runs = plans[stage]
                ws = wss[stage][runs[0][0]]
                shape = (batch_size, self.channels, image_size, image_size)
                if unet.lowres_cond:
                    if on_gpu:
                        img.record_stream(streams[stage])
                    self._lowres_conditioning(unet, img, image_size, ws, lowres_sample_noise_level, _noise, _seed, _sample_offset, stage)
                    for other in wss[stage].values():           # drawn once, then copied
                        if other is not ws:
                            other.lowres.copy_(ws.lowres)
                            unet.engine().prepare_lowres(other)
                loop = dict(noise_scheduler=noise_scheduler, noise_fn=_noise, seed=_seed, sample0=_sample_offset, stage=stage, use_graph=_use_graph,
                            solver=solvers[stage], **extras[stage])
                if len(runs) == 1 and runs[0][0] != 'table':
                    part = {} if init_starts[stage] is None else dict(steps=runs[0][1:3])          # (a run (a0, S) of the loop, like a plan's)
                    img = self._p_sample_loop(unet, shape, ws=ws, cond_scale=runs[0][3], begun=begun.get(stage), **loop, **rescaled[runs[0][0]], **part)
                else:
                    img = self._run_plan(unet, shape, runs, wss[stage], scale_tabs[stage], begun.get(stage), loop, rescaled)
                if on_gpu:
                    prev_done = streams[stage].record_event()
        pack_tokens = [] if (_noise is not None or _revalidated) else [(unet.engine(), unet.engine().pack_begin()) for unet in self.unets]
        if any(eng.pack_changed(tok) for eng, tok in pack_tokens):
            # the weights' values had changed behind the version counters (p.data updates): what was enqueued ran on stale packs
            if on_gpu:
                torch.cuda.synchronize(device)
            self._status_stages = []
            call_args["_revalidated"] = True
            return self.sample(**call_args)
        if self._status_stages:
            self._status_pending.append((prev_done, self._status_stages))
            self._status_stages = []
        if STRICT_STATUS and on_gpu and not _async:
            prev_done.synchronize()
            self._poll_status()
        if on_gpu:
            if _async:
                # pipelined use: the result is ready when ``done`` is (the caller synchronises / waits on it before touching the images)
                # per CALL: the event of this very call.  A later call on the OTHER lane does not wait for it -- capture it right after
                # the call that produced the tensor (it also travels on the tensor), or use wait_pending_samples() to cover every lane
                self.last_sample_done = prev_done
                self._lane_done[lane] = prev_done
                if not return_pil_images:
                    img.sample_done = prev_done
                    return img
            caller_stream.wait_event(prev_done)              # (_async with PIL images: the device -> host copy below runs on the caller's stream)
            img.record_stream(caller_stream)
        if not return_pil_images:
            return img
        pil = _to_pil_images(img)
        self.check_device_status()
        return pil

    def _run_plan(self, unet: Unet, shape, runs, workspaces, scales, begun, loop, rescaled):
        """A stage whose guidance plan has several runs, or reads its scales from a table: every run on the workspace of
        its kind, x / the history / the step index handed over at the run boundaries, one noise stream (``begun``: the stage_begin of the first
        run's workspace, issued here for injected noise -- one x_T and one draw per step, whatever workspaces the stage visits) -> the image."""
        first = workspaces[runs[0][0]]
        begin = {k: loop[k] for k in ('noise_scheduler', 'stage', 'solver', 'inpaint', 'objective') if k in loop}
        if 'init' in loop:                                       # the first run starts at step a0 (and selects the state of a 'dpmpp_2m' loop by it)
            begin['start'] = runs[0][1]
        if begun is None:
            begun = self._stage_begin(unet, shape, ws=first, noise_fn=loop['noise_fn'], seed=loop['seed'], sample0=loop['sample0'], **begin,
                                      **({'init': loop['init']} if 'init' in loop else {}))
        st0, noise_dev = begun
        states = {runs[0][0]: st0}
        for kind, ws in workspaces.items():
            if ws is not first:
                states[kind] = S.stage_attach(unet, shape, ws=ws, first=st0, max_states=MAX_SOLVER_STATES, **begin)
        n_steps = runs[-1][2]
        img = prev = None
        for i, (kind, a, b, scale) in enumerate(runs):
            if prev is not None:
                S.stage_handover(states[prev], workspaces[prev], states[kind], workspaces[kind], shape[0], n_steps - 1 - a)
            img = self._p_sample_loop(unet, shape, ws=workspaces[kind], cond_scale=1. if kind == 'table' else scale, begun=(states[kind], noise_dev),
                                      steps=(a, b), scale_tab=scales if kind == 'table' else None, finalize=i == len(runs) - 1, **loop, **rescaled[kind])
            prev = kind
        return img

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
