"""Noise schedule with the reference's class name and buffers (minimagen/diffusion_model.py)."""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn


class GaussianDiffusion(nn.Module):
    """Linear-beta DDPM schedule.  The twelve tables are computed in fp64 and stored as fp32
    non-persistent buffers exactly as diffusion_model.py:28-66 does, so every look-up value is
    bit-identical to the reference's.  On the sampling path the per-timestep arithmetic that consumes them
    (predict_start_from_noise / q_posterior / q_sample) runs inside the HIP sampler kernels; the methods of the
    same names below are the tensor forms of the class API."""

    def __init__(self, *, timesteps: int):
        super().__init__()
        assert not timesteps < 20, f'timsteps must be at least 20'
        self.num_timesteps = timesteps
        scale = 1000 / timesteps
        betas = torch.linspace(scale * 0.0001, scale * 0.02, timesteps, dtype=torch.float64)
        alphas = 1. - betas
        alphas_cumprod = torch.cumprod(alphas, dim=0)
        alphas_cumprod_prev = F.pad(alphas_cumprod[:-1], (1, 0), value=1.)
        reg = lambda name, val: self.register_buffer(name, val.to(torch.float32), persistent=False)
        reg('betas', betas)
        reg('alphas_cumprod', alphas_cumprod)
        reg('alphas_cumprod_prev', alphas_cumprod_prev)
        reg('sqrt_alphas_cumprod', torch.sqrt(alphas_cumprod))
        reg('sqrt_one_minus_alphas_cumprod', torch.sqrt(1. - alphas_cumprod))
        reg('log_one_minus_alphas_cumprod', torch.log(1. - alphas_cumprod))
        reg('sqrt_recip_alphas_cumprod', torch.sqrt(1. / alphas_cumprod))
        reg('sqrt_recipm1_alphas_cumprod', torch.sqrt(1. / alphas_cumprod - 1))
        posterior_variance = betas * (1. - alphas_cumprod_prev) / (1. - alphas_cumprod)
        reg('posterior_variance', posterior_variance)
        reg('posterior_log_variance_clipped', torch.log(posterior_variance.clamp(min=1e-20)))
        reg('posterior_mean_coef1', betas * torch.sqrt(alphas_cumprod_prev) / (1. - alphas_cumprod))
        reg('posterior_mean_coef2', (1. - alphas_cumprod_prev) * torch.sqrt(alphas) / (1. - alphas_cumprod))
        # host copies of the two q_sample tables (same fp32 values): the sampler reads one scalar of each per stage, and reading it from
        # the device buffer would synchronise the host with that stage's stream -- i.e. with the previous call still running on it
        self._host_sqrt_alphas_cumprod = self.sqrt_alphas_cumprod.tolist()
        self._host_sqrt_one_minus_alphas_cumprod = self.sqrt_one_minus_alphas_cumprod.tolist()

    def _get_times(self, batch_size: int, noise_level: float, *, device) -> torch.Tensor:
        """diffusion_model.py:68-69"""
        return torch.full((batch_size,), int(self.num_timesteps * noise_level), device=device, dtype=torch.long)

    def _sample_random_times(self, batch_size: int, *, device) -> torch.Tensor:
        return torch.randint(0, self.num_timesteps, (batch_size,), device=device, dtype=torch.long)

    def _get_sampling_timesteps(self, batch: int, *, device):
        """diffusion_model.py:81-87"""
        return [torch.full((batch,), i, device=device, dtype=torch.long) for i in reversed(range(self.num_timesteps))]

    def _abar64(self) -> torch.Tensor:
        """alphas_cumprod in fp64, from the betas as __init__ builds them"""
        scale = 1000 / self.num_timesteps
        betas = torch.linspace(scale * 0.0001, scale * 0.02, self.num_timesteps, dtype=torch.float64)
        return torch.cumprod(1. - betas, dim=0)

    @staticmethod
    def _known_columns64(a: torch.Tensor) -> torch.Tensor:
        """float64[S][2], the inpainting columns 6 and 7 of a coefficient table whose rows sit at abar = ``a``: sqrt(abar_{k-1}) and
        sqrt(1 - abar_{k-1}) with abar_{-1} = 1 -- the level the known pixels are re-imposed at behind step k; row 0 is exactly (1, 0)"""
        ap = F.pad(a[:-1], (1, 0), value=1.)
        return torch.stack((torch.sqrt(ap), torch.sqrt(1. - ap)), dim=1)

    def known_start_coefs(self):
        """(a, b) = (sqrt(abar_{T-1}), sqrt(1 - abar_{T-1})) as fp32 values: the level of x_T, where the known region of an inpainting call
        is imposed first (blend 0).  Every step count and sampler starts at the trained timestep T-1."""
        a = self._abar64()[-1]
        return float(torch.sqrt(a).to(torch.float32)), float(torch.sqrt(1. - a).to(torch.float32))

    def init_start_coefs(self, steps: int = None, start: int = 0):
        """(a, b) = (sqrt(abar_tau), sqrt(1 - abar_tau)) as fp32 values at tau = tau_{S-1-start}, the trained timestep of the first step a loop
        of S = ``steps`` steps (None: T, the default loop) executes when it skips its first ``start`` steps: the level an init image is noised
        to (Imagen.sample(init_images=)).  fp64 from the betas, rounded once; ``start`` = 0 is known_start_coefs() -- and ``start`` >= 1 is
        columns 6 and 7 of row S - start of the ``known`` table, the level behind step S - start."""
        T = self.num_timesteps
        S = T if steps is None else int(steps)
        tau = torch.arange(T) if steps is None else self.sampling_timestep_map(S)
        if isinstance(start, bool) or not isinstance(start, int) or not 0 <= start < S:
            raise ValueError(f'start must be an int in [0, {S - 1}] for a loop of {S} steps, got {start!r}')
        a = self._abar64()[int(tau[S - 1 - start])]
        return float(torch.sqrt(a).to(torch.float32)), float(torch.sqrt(1. - a).to(torch.float32))

    OBJECTIVES = ('noise', 'x_start', 'v')

    @classmethod
    def _check_objective(cls, objective):
        if objective not in cls.OBJECTIVES:
            raise ValueError(f'objective must be one of {cls.OBJECTIVES}, got {objective!r}')

    @classmethod
    def _objective_columns64(cls, a: torch.Tensor, objective: str):
        """float64[S][2] or None ('noise': the table's own columns stay): columns 0 and 1 of a coefficient table whose rows sit at abar = ``a``,
        so that x0 = c0 x_t - c1 pred for a U-Net that predicts ``objective`` -- 'v': (sqrt(abar), sqrt(1 - abar));
        'x_start': exactly (0, -1), 0 x_t - (-1) pred being pred to the bit"""
        cls._check_objective(objective)
        if objective == 'noise':
            return None
        if objective == 'v':
            return torch.stack((torch.sqrt(a), torch.sqrt(1. - a)), dim=1)
        return torch.stack((torch.zeros_like(a), -torch.ones_like(a)), dim=1)

    def sampler_coef_table(self, known: bool = False, objective: str = 'noise') -> torch.Tensor:
        """[T][8] table consumed by mi_cfg_x0_fwd / mi_posterior_fwd: per-timestep scalars gathered from the
        buffers above; column 4 is [t != 0] * exp(0.5 * posterior_log_variance_clipped) (Imagen.py:364-370).
        ``known``: plus the inpainting columns 6 and 7 (fp64 from the betas, rounded once); without it they are zero.
        ``objective``: what the U-Net predicts -- 'v' / 'x_start' replace columns 0 and 1 (_objective_columns64: fp64 from the betas, rounded
        once); 'noise' is the table as it was before the argument existed."""
        T = self.num_timesteps
        tab = torch.zeros(T, 8, dtype=torch.float32)
        cpu = lambda v: v.detach().to('cpu', torch.float32)
        tab[:, 0] = cpu(self.sqrt_recip_alphas_cumprod)
        tab[:, 1] = cpu(self.sqrt_recipm1_alphas_cumprod)
        tab[:, 2] = cpu(self.posterior_mean_coef1)
        tab[:, 3] = cpu(self.posterior_mean_coef2)
        nonzero = torch.ones(T)
        nonzero[0] = 0.
        tab[:, 4] = nonzero * (0.5 * cpu(self.posterior_log_variance_clipped)).exp()
        if known:
            tab[:, 6:8] = self._known_columns64(self._abar64()).to(torch.float32)
        cols = self._objective_columns64(self._abar64(), objective)
        if cols is not None:
            tab[:, 0:2] = cols.to(torch.float32)
        return tab

    # ---- sampling in S <= T steps over a subsequence of the trained timesteps (not in the reference; DESIGN.md "Fewer sampling steps")
    SAMPLERS = ('ddpm', 'ddim', 'dpmpp_2m')

    def sampling_timestep_map(self, steps: int) -> torch.Tensor:
        """tau int64[S]: tau_k = round(k (T-1) / (S-1)) in integer arithmetic -- contains 0 and T-1, strictly increasing, arange(T) for S = T"""
        T, S = self.num_timesteps, int(steps)
        if not 2 <= S <= T:
            raise ValueError(f'sample_steps must be in [2, {T}] for a schedule of {T} timesteps, got {steps}')
        return torch.tensor([(2 * k * (T - 1) + (S - 1)) // (2 * (S - 1)) for k in range(S)], dtype=torch.int64)

    def _sampler_tables64(self, steps: int, sampler: str = 'ddpm', eta: float = None, known: bool = False, objective: str = 'noise', start: int = 0):
        """sampler_tables before the rounding to fp32: (tau int64[S], abar float64[S], coef float64[S][8])"""
        self._check_objective(objective)
        if sampler not in self.SAMPLERS:
            raise ValueError(f'sampler must be one of {self.SAMPLERS}, got {sampler!r}')
        if eta is not None and sampler != 'ddim':
            raise ValueError("sampler_eta goes with sampler='ddim' only")
        eta = 1. if sampler == 'ddpm' else (0. if eta is None else float(eta))
        if not 0. <= eta <= 1.:
            raise ValueError(f'sampler_eta must be in [0, 1], got {eta}')
        tau = self.sampling_timestep_map(steps)
        T, S = self.num_timesteps, tau.numel()
        if isinstance(start, bool) or not isinstance(start, int) or not 0 <= start < S:
            raise ValueError(f'start must be an int in [0, {S - 1}] for a loop of {S} steps, got {start!r}')
        scale = 1000 / T
        betas = torch.linspace(scale * 0.0001, scale * 0.02, T, dtype=torch.float64)        # as __init__, kept in fp64
        a = torch.cumprod(1. - betas, dim=0)[tau]
        ap = F.pad(a[:-1], (1, 0), value=1.)
        tab = torch.zeros(S, 8, dtype=torch.float64)
        tab[:, 0] = torch.sqrt(1. / a)
        tab[:, 1] = torch.sqrt(1. / a - 1)
        if sampler != 'dpmpp_2m':
            # Song et al. 2021 (DDIM), eq. 12 and 16, written on x0: x_{k-1} = sqrt(ap) x0 + sqrt(1 - ap - sigma^2) eps + sigma z
            sigma = eta * torch.sqrt((1. - ap) / (1. - a)) * torch.sqrt(1. - a / ap)
            tab[:, 3] = torch.sqrt((1. - ap - sigma ** 2).clamp(min=0.)) / torch.sqrt(1. - a)
            tab[:, 2] = torch.sqrt(ap) - tab[:, 3] * torch.sqrt(a)
            tab[:, 4] = sigma
            tab[0, 4] = 0.
        else:
            # Lu et al. 2022 (DPM-Solver++), Algorithm 2 (2M, data prediction) on the thresholded x0
            al, sg = torch.sqrt(a), torch.sqrt(1. - a)
            lam = torch.log(al / sg)
            tab[0, 2] = 1.                                   # the last step returns x0
            for k in range(1, S):
                h = lam[k - 1] - lam[k]
                m = al[k - 1] * (1. - torch.exp(-h))
                tab[k, 3] = sg[k - 1] / sg[k]
                if k == S - 1 or k == S - 1 - start:         # first step (executed: a loop that skips ``start`` steps): no history yet (DPM-Solver++ 1 = DDIM)
                    tab[k, 2] = m
                else:
                    r = (lam[k] - lam[k + 1]) / h
                    tab[k, 2] = m * (1. + 1. / (2. * r))
                    tab[k, 5] = -m / (2. * r)
        if known:
            tab[:, 6:8] = self._known_columns64(a)
        cols = self._objective_columns64(a, objective)
        if cols is not None:
            tab[:, 0:2] = cols
        return tau, a, tab

    def sampler_tables(self, steps: int, sampler: str = 'ddpm', eta: float = None, known: bool = False, objective: str = 'noise', start: int = 0):
        """(tau int64[S], coef float32[S][8]) for ``steps`` sampling steps over the trained timesteps tau: row k of ``coef`` is the step at
        timestep tau_k (the sampler walks k = S-1 .. 0).  With cN = column N (the naming of DESIGN.md section 14 and the C header): x0 = c0 x - c1 eps, then
        x' = c2 x0 + c3 x + c5 x0_prev + c4 z with the thresholded x0 of this and of the previous step.  'ddpm' is 'ddim' with eta = 1 (the reference's ancestral step when
        S = T); 'dpmpp_2m' is deterministic.  Everything in fp64 from the betas, rounded to fp32 once.  ``known``: plus c6 = sqrt(abar_{tau_{k-1}}) and
        c7 = sqrt(1 - abar_{tau_{k-1}}), the level an inpainting call re-imposes its known pixels at behind step k (row 0: exactly 1 and 0);
        without it columns 6 and 7 are zero and the table is what it was before the flag existed.  ``objective`` = 'v' / 'x_start': c0 and c1 turn
        that prediction into x0 (sampler_coef_table); the solvers work on x0 and x only, so columns 2 .. 7 do not depend on it.
        ``start`` = a0 > 0: the loop skips its first a0 steps (an init image), so row S-1-a0 is the first one executed --
        for 'dpmpp_2m' that row gets the first-order coefficients (no history yet: c2 = m, c5 = 0); every other row, every other sampler and
        ``start`` = 0 are bit-identical to the table without the argument."""
        tau, _, tab = self._sampler_tables64(steps, sampler, eta, known, objective, start)
        return tau, tab.to(torch.float32)

    def loss_weight_table(self, objective: str, min_snr_gamma: float = None) -> torch.Tensor:
        """float32[T], the per-timestep weight of the training loss of a U-Net that predicts ``objective``, in fp64 from the betas and rounded
        once.  Min-SNR-gamma (Hang et al. 2023) with snr = abar / (1 - abar) and c = min(snr, gamma): 'noise' c / snr, 'x_start' c,
        'v' c / (snr + 1).  Where snr is exactly 0 (abar underflows: T = 20) 'noise' takes its limit 1, the other two are 0.
        ``min_snr_gamma`` None: all ones."""
        self._check_objective(objective)
        if min_snr_gamma is None:
            return torch.ones(self.num_timesteps, dtype=torch.float32)
        gamma = float(min_snr_gamma)
        if not gamma > 0.:
            raise ValueError(f'min_snr_gamma must be positive, got {min_snr_gamma!r}')
        a = self._abar64()
        snr = a / (1. - a)
        c = snr.clamp(max=gamma)
        if objective == 'noise':
            w = torch.where(snr > 0., c / snr.clamp(min=torch.finfo(torch.float64).tiny), torch.ones_like(snr))
        elif objective == 'x_start':
            w = c
        else:
            w = c / (snr + 1.)
        return w.to(torch.float32)

    # ---- the per-timestep helpers of the reference's public API (diffusion_model.py:89-162).  The sampling hot path has them fused
    # into the HIP sampler kernels (mi_lowres_augment, mi_cfg_x0_fwd, mi_posterior_fwd); these tensor forms serve callers of the class
    # API and the training loss (Imagen.forward), on whatever device the tables live, and are differentiable.
    @staticmethod
    def _at(table: torch.Tensor, t: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
        """table[t] broadcast over an image batch: (b,) -> (b, 1, 1, 1) (helpers.extract, helpers.py:48-59)"""
        return table.gather(-1, t).reshape(t.shape[0], *((1,) * (like.dim() - 1)))

    def q_sample(self, x_start: torch.Tensor, t: torch.Tensor, noise: torch.Tensor = None) -> torch.Tensor:
        """x_t = sqrt(abar_t) x_0 + sqrt(1 - abar_t) eps (diffusion_model.py:127-147)"""
        if noise is None:
            noise = torch.randn_like(x_start)
        return self._at(self.sqrt_alphas_cumprod, t, x_start) * x_start + self._at(self.sqrt_one_minus_alphas_cumprod, t, x_start) * noise

    def q_posterior(self, x_start: torch.Tensor, x_t: torch.Tensor, t: torch.Tensor):
        """mean, variance and clipped log-variance of q(x_{t-1} | x_t, x_0) (diffusion_model.py:89-125)"""
        mean = self._at(self.posterior_mean_coef1, t, x_t) * x_start + self._at(self.posterior_mean_coef2, t, x_t) * x_t
        return mean, self._at(self.posterior_variance, t, x_t), self._at(self.posterior_log_variance_clipped, t, x_t)

    def predict_start_from_noise(self, x_t: torch.Tensor, t: torch.Tensor, noise: torch.Tensor) -> torch.Tensor:
        """x_0 = sqrt(1 / abar_t) x_t - sqrt(1 / abar_t - 1) eps (diffusion_model.py:149-162)"""
        return self._at(self.sqrt_recip_alphas_cumprod, t, x_t) * x_t - self._at(self.sqrt_recipm1_alphas_cumprod, t, x_t) * noise

    def calculate_v(self, x_start: torch.Tensor, t: torch.Tensor, noise: torch.Tensor) -> torch.Tensor:
        """v = sqrt(abar_t) eps - sqrt(1 - abar_t) x_0 (Salimans & Ho 2022, appendix D)"""
        return self._at(self.sqrt_alphas_cumprod, t, x_start) * noise - self._at(self.sqrt_one_minus_alphas_cumprod, t, x_start) * x_start

    def predict_start_from_v(self, x_t: torch.Tensor, t: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
        """x_0 = sqrt(abar_t) x_t - sqrt(1 - abar_t) v"""
        return self._at(self.sqrt_alphas_cumprod, t, x_t) * x_t - self._at(self.sqrt_one_minus_alphas_cumprod, t, x_t) * v
