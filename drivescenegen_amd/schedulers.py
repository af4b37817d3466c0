"""``DDPMScheduler`` / ``DDIMScheduler`` with the diffusers-0.20.0 protocol DriveSceneGen uses, ``RePaintScheduler``
(scene completion with the same unconditional network) and ``DPMSolverMultistepScheduler`` (DPM-Solver++: the same network in
a fraction of the steps); diffusers 0.20.0 ships both next to the other two.

Reference call sites: /root/reference/DriveSceneGen/scripts/train.py:65 (``DDPMScheduler()``, all defaults),
training_pipeline.py:76 (``.num_train_timesteps`` as a direct attribute), training_pipeline.py:80 and
train.py:91 (``add_noise``), and ``set_timesteps`` / ``step`` inside the DDPMPipeline loop
(training_pipeline.py:26-32, generation.py:14-20).  DDIM is the BASELINE.json extension (configs[1], [3]).
Formulas: SURVEY.md App. A.3 / A.3b.

Host side (this file): the beta / alpha-bar tables, the integer timestep tables and the per-step fp32
scalars, computed with the same fp32 operation order as the reference so they are bit-identical.
Device side: the elementwise tensor math, in libdsg.so (dsg_add_noise / dsg_ddpm_step / dsg_ddim_step / dsg_repaint_step /
dsg_repaint_undo / dsg_dpmsolver_step; with ``thresholding=True``: dsg_dynthresh_scale + dsg_ddpm_step_thr / dsg_ddim_step_thr;
with ``prediction_type`` "sample" / "v_prediction": dsg_ddpm_step_pt / dsg_ddim_step_pt, and dsg_add_noise_target for the
training target).

Which config values a class runs is ONE table per class, ``_choices``: DDPM and DDIM take the three beta schedules, the three
prediction types and the three timestep spacings of diffusers 0.20.0 (DDIM also ``rescale_betas_zero_snr``); RePaint and
DPM-Solver++ stay on linear betas and epsilon prediction.

Layout: ``_SchedulerBase`` holds what all four classes share (config handling, the tables, ``add_noise``, config I/O, the
memo helper); ``_Thresholding`` is the dynamic-thresholding mixin of DDPM and DDIM; ``_NoiseSource`` is the device-noise switch
of RePaint and DPM-Solver.  Every ``step`` that takes a noise tensor resolves it through ``_resolve_noise`` -- one place that
decides where the noise comes from, checks its shape and makes it contiguous fp32 on the sample's device.
"""
from __future__ import annotations

import json
import math
import os
from types import SimpleNamespace
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from .unet import FrozenConfig


class SchedulerOutput(SimpleNamespace):
    pass


def _randn_like_reference(shape, generator, device, dtype):
    """diffusers ``randn_tensor``: a CPU generator samples on CPU and the result is moved (App. A.4)."""
    if generator is not None and generator.device.type == "cpu" and torch.device(device).type != "cpu":
        return torch.randn(shape, generator=generator, device="cpu", dtype=dtype).to(device)
    return torch.randn(shape, generator=generator, device=device, dtype=dtype)


class HostNoise:
    """A step's variance noise in PINNED host memory, read in place by the step kernel (one pass over PCIe) instead of being
    copied to the device first -- what ``DDPMPipeline`` hands to ``step(..., variance_noise=...)`` when the caller's generator
    lives on the CPU (training_pipeline.py:26-32).  `consumed` is recorded on the launch stream behind the kernel that read
    the buffer; its owner waits for it before writing the buffer again."""

    def __init__(self, tensor):
        if tensor.is_cuda or not tensor.is_contiguous() or tensor.dtype != torch.float32 or not tensor.is_pinned():
            raise ValueError("HostNoise: a contiguous pinned fp32 host tensor is required")
        self.tensor = tensor
        self.consumed = None
        # the address the KERNEL reads: asked of the runtime, not assumed equal to the host address (torch's host-register
        # configuration of the pinned allocator maps the two apart)
        import ctypes
        dev = ctypes.c_void_p()
        _lib.check(_lib.load().dsg_host_device_pointer(tensor.data_ptr(), ctypes.byref(dev)))
        self.device_ptr = dev.value

    @property
    def shape(self):
        return self.tensor.shape

    def wait_consumed(self):
        if self.consumed is not None:
            self.consumed.synchronize()


class _StepNoise(NamedTuple):
    """What a step kernel is told about its noise: `ptr` to read it from (None: none, or made in the kernel from the Philox
    tensor (`seed`, `offset`)), `tensor` to keep alive until the launch, `host` to tell when the kernel has read it."""
    ptr: Optional[int] = None
    tensor: Optional[torch.Tensor] = None
    host: Optional[HostNoise] = None
    seed: int = 0
    offset: int = 0


def _resolve_noise(variance_noise, sample, generator, source=None):
    """Where one step's noise comes from, in this order: the caller's ``variance_noise`` (a ``HostNoise``, read in place, or a
    tensor); the next Philox tensor of `source` (a ``_NoiseSource`` in device mode), made inside the kernel; a draw from
    `generator`, as diffusers makes it.  A tensor is checked against the sample's shape and handed over contiguous, fp32 and on
    the sample's device: the kernels read `sample.numel()` floats from the pointer."""
    shape = tuple(sample.shape)
    if variance_noise is None:
        if source is not None and source.noise_mode == "device":
            return _StepNoise(seed=source.noise_seed, offset=source._next_offset())
        variance_noise = _randn_like_reference(shape, generator, sample.device, sample.dtype)
    if tuple(variance_noise.shape) != shape:
        raise ValueError(f"variance_noise has shape {tuple(variance_noise.shape)}, the sample {shape}")
    if isinstance(variance_noise, HostNoise):        # pinned host buffer: the kernel reads it in place
        return _StepNoise(ptr=variance_noise.device_ptr, host=variance_noise)
    z = variance_noise.to(sample.device, torch.float32).contiguous()
    return _StepNoise(ptr=_lib.ptr(z), tensor=z)


def _record_consumed(noise, device):
    """Behind the launch that read `noise` (on `device`'s current stream): lets a ``HostNoise``'s owner reuse the buffer."""
    if noise.host is not None:
        noise.host.consumed = torch.cuda.Event()
        noise.host.consumed.record(torch.cuda.current_stream(device))


class _SchedulerBase:
    """What the four schedulers share: config handling, the beta / alpha-bar tables, ``add_noise``, config I/O."""
    config_name = "scheduler_config.json"
    order = 1
    _defaults = {}
    _choices = {}           # config key -> the values this class runs; any other value raises (a key not listed is free)
    _named_by_diffusers = ()    # keys of _choices whose unknown values diffusers itself rejects with a ValueError

    def __init__(self, **kwargs):
        cfg = dict(self._defaults)
        unknown = set(kwargs) - set(cfg)
        if unknown:
            raise TypeError(f"{self._class_name}: unexpected arguments {sorted(unknown)}")
        cfg.update(kwargs)
        for key, allowed in self._choices.items():
            v = cfg[key]
            if isinstance(v, bool) != isinstance(allowed[0], bool) or v not in allowed:
                error = ValueError if key in self._named_by_diffusers else NotImplementedError
                raise error(f"{self._class_name}: {key}={v!r} is outside the DriveSceneGen path "
                            f"(supported: {allowed[0] if len(allowed) == 1 else allowed!r})")
        self._check_extra(cfg)
        self.config = FrozenConfig(**cfg)
        n = cfg["num_train_timesteps"]
        self.betas = self._betas(cfg)
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.one = torch.tensor(1.0)
        self.init_noise_sigma = 1.0
        self.num_inference_steps = None
        self.custom_timesteps = False
        self.timesteps = torch.from_numpy(np.arange(0, n)[::-1].copy())
        self._dev_tables = {}
        self._scalar_cache = {}
        self._snr_tables = {}

    def _check_extra(self, cfg):
        """The class's own refusals, on the merged config."""

    def _betas(self, cfg):
        """The fp32 beta table of ``beta_schedule``, in diffusers' operation order."""
        n, schedule = cfg["num_train_timesteps"], cfg["beta_schedule"]
        if schedule == "linear":
            return torch.linspace(cfg["beta_start"], cfg["beta_end"], n, dtype=torch.float32)
        if schedule == "scaled_linear":
            return torch.linspace(cfg["beta_start"] ** 0.5, cfg["beta_end"] ** 0.5, n, dtype=torch.float32) ** 2
        if schedule == "squaredcos_cap_v2":     # (Nichol & Dhariwal's cosine alpha-bar, in Python doubles)
            def alpha_bar(t):
                return math.cos((t + 0.008) / 1.008 * math.pi / 2) ** 2
            return torch.tensor([min(1 - alpha_bar((i + 1) / n) / alpha_bar(i / n), 0.999) for i in range(n)], dtype=torch.float32)
        raise NotImplementedError(f"{self._class_name}: beta_schedule={schedule!r}")

    @staticmethod
    def _memo(cache, key, make):
        """cache[key], made by `make()` on first use (the per-step scalars are a dozen 0-d tensor operations, ~50 us of host
        time per denoising step otherwise)."""
        hit = cache.get(key)
        if hit is None:
            hit = cache[key] = make()
        return hit

    # training_pipeline.py:76 reads this attribute directly
    @property
    def num_train_timesteps(self):
        return self.config.num_train_timesteps

    def __len__(self):
        return self.config.num_train_timesteps

    def scale_model_input(self, sample, timestep=None):
        return sample

    # ---- add_noise (training_pipeline.py:80; train.py:91 with an HWC image and timesteps=[1]) ----
    def _sqrt_tables(self, device):
        key = str(device)
        if key not in self._dev_tables:
            ac = self.alphas_cumprod
            self._dev_tables[key] = ((ac ** 0.5).to(device), ((1 - ac) ** 0.5).to(device))
        return self._dev_tables[key]

    def add_noise(self, original_samples, noise, timesteps):
        x0 = original_samples
        if not x0.is_cuda:
            raise RuntimeError("DDPMScheduler.add_noise runs on the MI355X HIP engine only (got a CPU tensor)")
        if x0.dtype != torch.float32:
            raise RuntimeError("add_noise: fp32 only")
        sa_t, sb_t = self._sqrt_tables(x0.device)
        t = timesteps.to(x0.device).flatten()
        sa, sb = sa_t[t].contiguous(), sb_t[t].contiguous()
        n = t.numel()
        if x0.dim() == 0 or (n != 1 and n != x0.shape[0]):
            raise ValueError("add_noise: timesteps must have one entry per leading-dim sample (or one entry)")
        if n == 1:
            per = x0.numel()
        else:
            per = x0.numel() // n
        x0c, nz = x0.contiguous(), noise.to(x0.device, x0.dtype).contiguous()
        out = torch.empty_like(x0c)
        with torch.cuda.device(x0.device):
            _lib.check(_lib.load().dsg_add_noise(_lib.ptr(x0c), _lib.ptr(nz), _lib.ptr(sa), _lib.ptr(sb),
                                                _lib.ptr(out), n, per, _lib.stream_ptr(x0.device)))
        return out

    def add_noise_device(self, original_samples, timesteps, seed: int, offset: int):
        """(noisy, noise): the training step's ``noise = torch.randn(shape).to(device)`` (training_pipeline.py:72) and
        ``add_noise(x0, noise, t)`` (:80) as ONE pass of a library kernel -- the noise is a counter-based Philox4x32-10 /
        Box-Muller stream named by (seed, offset) (``dsg_add_noise_philox``, include/dsg.h), not the host generator's:
        opt-in (``train_steps(..., noise="device")``), for throughput.  `noisy` is bitwise ``add_noise(x0, noise, t)``."""
        x0 = original_samples
        if not x0.is_cuda or x0.dtype != torch.float32:
            raise RuntimeError("DDPMScheduler.add_noise_device runs on the MI355X HIP engine only (an fp32 GPU tensor)")
        sa_t, sb_t = self._sqrt_tables(x0.device)
        t = timesteps.to(x0.device).flatten()
        n = t.numel()
        if x0.dim() == 0 or (n != 1 and n != x0.shape[0]):
            raise ValueError("add_noise_device: timesteps must have one entry per leading-dim sample (or one entry)")
        sa, sb = sa_t[t].contiguous(), sb_t[t].contiguous()
        x0c = x0.contiguous()
        noisy, noise = torch.empty_like(x0c), torch.empty_like(x0c)
        with torch.cuda.device(x0.device):
            _lib.check(_lib.load().dsg_add_noise_philox(_lib.ptr(x0c), _lib.ptr(sa), _lib.ptr(sb), _lib.ptr(noisy),
                                                       _lib.ptr(noise), n, x0c.numel() // n, int(seed) & (2 ** 64 - 1),
                                                       int(offset) & (2 ** 64 - 1), _lib.stream_ptr(x0.device)))
        return noisy, noise

    # ---- the velocity target of a v-predicting network ------------------------------------------------------------
    def _noise_target(self, who, x0, noise, timesteps, want_noisy, seed=0, offset=0):
        """(noisy or None, target) of ``dsg_add_noise_target`` (`noise` a tensor) / ``dsg_add_noise_target_philox`` (`noise`
        None: the Philox tensor (seed, offset)): one pass over (x0, noise); the timestep rules are ``add_noise``'s."""
        if not x0.is_cuda or x0.dtype != torch.float32:
            raise RuntimeError(f"DDPMScheduler.{who} runs on the MI355X HIP engine only (an fp32 GPU tensor)")
        sa_t, sb_t = self._sqrt_tables(x0.device)
        t = timesteps.to(x0.device).flatten()
        n = t.numel()
        if x0.dim() == 0 or (n != 1 and n != x0.shape[0]):
            raise ValueError(f"{who}: timesteps must have one entry per leading-dim sample (or one entry)")
        sa, sb = sa_t[t].contiguous(), sb_t[t].contiguous()
        x0c = x0.contiguous()
        noisy, target = (torch.empty_like(x0c) if want_noisy else None), torch.empty_like(x0c)
        lib, st, per = _lib.load(), _lib.stream_ptr(x0.device), x0c.numel() // n
        with torch.cuda.device(x0.device):
            if noise is not None:
                if tuple(noise.shape) != tuple(x0.shape):
                    raise ValueError(f"{who}: noise has shape {tuple(noise.shape)}, the sample {tuple(x0.shape)}")
                nz = noise.to(x0.device, x0.dtype).contiguous()
                _lib.check(lib.dsg_add_noise_target(_lib.ptr(x0c), _lib.ptr(nz), _lib.ptr(sa), _lib.ptr(sb), _lib.ptr(noisy),
                                                    _lib.ptr(target), n, per, st))
            else:
                _lib.check(lib.dsg_add_noise_target_philox(_lib.ptr(x0c), _lib.ptr(sa), _lib.ptr(sb), _lib.ptr(noisy),
                                                           _lib.ptr(target), n, per, int(seed) & (2 ** 64 - 1),
                                                           int(offset) & (2 ** 64 - 1), st))
        return noisy, target

    def get_velocity(self, sample, noise, timesteps):
        """diffusers' ``get_velocity``: v = sqrt(abar_t)*noise - sqrt(1 - abar_t)*sample, the target of a network trained with
        ``prediction_type="v_prediction"`` (Salimans & Ho, 2022)."""
        return self._noise_target("get_velocity", sample, noise, timesteps, want_noisy=False)[1]

    def add_noise_velocity(self, original_samples, noise, timesteps):
        """(noisy, velocity): ``add_noise`` and ``get_velocity`` as ONE pass over (x0, noise); both bitwise the single calls."""
        return self._noise_target("add_noise_velocity", original_samples, noise, timesteps, want_noisy=True)

    def add_noise_velocity_device(self, original_samples, timesteps, seed: int, offset: int):
        """(noisy, velocity) for the Philox noise tensor (seed, offset) of ``add_noise_device``, which is made in the kernel and
        not written: `noisy` is bitwise ``add_noise_device``'s, `velocity` bitwise ``get_velocity`` of that noise."""
        return self._noise_target("add_noise_velocity_device", original_samples, None, timesteps, True, seed, offset)

    # ---- min-SNR-gamma loss weights (Hang et al., "Efficient Diffusion Training via Min-SNR Weighting Strategy", 2023) ------
    def snr_weights(self, gamma: float, device=None):
        """The per-timestep loss weight, fp32 [num_train_timesteps] on `device` (cached; index it with the step's timesteps):
        min(snr, gamma) / snr for an epsilon-predicting network, / (snr + 1) for v-prediction, min(snr, gamma) itself for
        sample prediction; snr = (sqrt(abar) / sqrt(1 - abar))^2 in fp32."""
        gamma = float(gamma)
        if not gamma > 0.0:
            raise ValueError(f"{self._class_name}.snr_weights: gamma={gamma!r} must be positive")
        pred = self.config.get("prediction_type", "epsilon")

        def make():
            ac = self.alphas_cumprod
            snr = (torch.sqrt(ac) / torch.sqrt(1 - ac)) ** 2
            w = torch.clamp(snr, max=gamma)
            if pred == "epsilon":
                if bool((snr == 0).any()):
                    raise ValueError(f"{self._class_name}.snr_weights: a zero-terminal-SNR table has no epsilon weight (0 / 0); "
                                     "train it with prediction_type='v_prediction' or 'sample'")
                w = w / snr
            elif pred == "v_prediction":
                w = w / (snr + 1)
            return w.to(device) if device is not None else w
        return self._memo(self._snr_tables, (gamma, pred, str(device)), make)

    # ---- config I/O (App. A.5) ----------------------------------------------------------------------
    def save_pretrained(self, save_directory):
        os.makedirs(save_directory, exist_ok=True)
        cfg = {"_class_name": self._class_name, "_diffusers_version": "0.20.0"}
        cfg.update(self.config.to_dict())
        with open(os.path.join(save_directory, self.config_name), "w") as f:
            json.dump(cfg, f, indent=2, sort_keys=True)
            f.write("\n")

    @classmethod
    def from_pretrained(cls, path, subfolder=None, **_unused):
        d = os.path.join(path, subfolder) if subfolder else path
        with open(os.path.join(d, cls.config_name)) as f:
            cfg = json.load(f)
        cfg = {k: v for k, v in cfg.items() if k in cls._defaults}
        return cls(**cfg)

    @classmethod
    def from_config(cls, config, **overrides):
        """A scheduler of THIS class from another's config: keys this class lacks are dropped (diffusers' swap idiom,
        ``pipe.scheduler = Other.from_config(pipe.scheduler.config)``); `overrides` replace or add entries, as in diffusers."""
        cfg = config.to_dict() if hasattr(config, "to_dict") else dict(config)
        cfg = {k: v for k, v in cfg.items() if k in cls._defaults}
        cfg.update(overrides)
        return cls(**cfg)


class _Thresholding:
    """Dynamic thresholding (diffusers' ``thresholding`` / ``dynamic_thresholding_ratio`` / ``sample_max_value``) for the two
    classes that run it, DDPMScheduler and DDIMScheduler."""

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self._rank_cache = {}           # (per, q) -> (k_lo, k_hi, w) of the thresholding quantile
        self._thr_buffers = {}          # (device, n) -> (workspace, workspace bytes, s [n])

    def _check_thresholding(self, cfg):
        """Called from ``_check_extra`` of a class whose config has the three keys."""
        if not isinstance(cfg["thresholding"], (bool, np.bool_)):
            raise ValueError(f"{self._class_name}: thresholding={cfg['thresholding']!r} is not a bool")
        q, m = cfg["dynamic_thresholding_ratio"], cfg["sample_max_value"]
        if isinstance(q, bool) or not isinstance(q, (int, float, np.integer, np.floating)) or not 0.0 <= q <= 1.0:
            raise ValueError(f"{self._class_name}: dynamic_thresholding_ratio={q!r} is outside [0, 1]")
        if isinstance(m, bool) or not isinstance(m, (int, float, np.integer, np.floating)) or not 1.0 <= m < float("inf"):
            raise ValueError(f"{self._class_name}: sample_max_value={m!r} is not a finite number >= 1")
        if cfg["thresholding"]:     # (dsg_dynthresh_scale ranks the epsilon form of p0; the tables it was checked on are these)
            for key in ("prediction_type", "beta_schedule", "timestep_spacing"):
                if cfg[key] != self._defaults[key]:
                    raise NotImplementedError(f"{self._class_name}: {key}={cfg[key]!r} with thresholding=True is outside the "
                                              f"DriveSceneGen path (supported: {self._defaults[key]!r})")

    def threshold_ranks(self, per: int):
        """(k_lo, k_hi, w) of the ``dynamic_thresholding_ratio`` quantile of `per` values, as torch.quantile forms them: the
        rank is the fp32 product q * (per - 1).  Memoised per (per, q)."""
        q = float(self.config.dynamic_thresholding_ratio)

        def make():
            rank = np.float32(q) * np.float32(per - 1)
            # (per - 1 above 2^24 may round UP on its way to fp32: no rank leaves the sample)
            k_lo = min(int(np.floor(rank)), per - 1)
            k_hi = min(int(np.ceil(rank)), per - 1)
            return k_lo, k_hi, float(rank - np.float32(k_lo)) if k_hi > k_lo else 0.0
        return self._memo(self._rank_cache, (int(per), q), make)

    def _threshold_scale(self, x, e, s):
        """The per-sample scale of the thresholded data prediction, device fp32 [N] (``dsg_dynthresh_scale``; include/dsg.h).
        The workspace and the result live in buffers cached per (device, N): the result is consumed by the step kernel
        enqueued right behind, on the same stream."""
        n = int(x.shape[0])
        per = x.numel() // n
        lib = _lib.load()
        key = (str(x.device), n)
        buf = self._thr_buffers.get(key)
        if buf is None:
            import ctypes
            nbytes = ctypes.c_size_t()
            _lib.check(lib.dsg_dynthresh_workspace_bytes(n, ctypes.byref(nbytes)))
            buf = self._thr_buffers[key] = (torch.empty(nbytes.value, dtype=torch.uint8, device=x.device), nbytes.value,
                                            torch.empty(n, dtype=torch.float32, device=x.device))
        ws, ws_bytes, scale = buf
        k_lo, k_hi, w = self.threshold_ranks(per)
        _lib.check(lib.dsg_dynthresh_scale(_lib.ptr(x), _lib.ptr(e), _lib.ptr(scale), n, per, s["sqrt_beta_prod_t"],
                                           s["sqrt_alpha_prod_t"], k_lo, k_hi, w, float(self.config.sample_max_value),
                                           _lib.ptr(ws), ws_bytes, _lib.stream_ptr(x.device)))
        return scale, per

    @staticmethod
    def _check_thresholded_inputs(who, sample, model_output):
        if sample.dim() < 2 or sample.numel() == 0 or sample.dtype != torch.float32 or model_output.dtype != torch.float32:
            raise ValueError(f"{who}: thresholding needs a non-empty fp32 [N, ...] sample")
        if tuple(model_output.shape) != tuple(sample.shape):
            raise ValueError(f"{who}: model output {tuple(model_output.shape)} != sample {tuple(sample.shape)}")


class DDPMScheduler(_Thresholding, _SchedulerBase):
    _class_name = "DDPMScheduler"
    _defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                     trained_betas=None, variance_type="fixed_small", clip_sample=True, prediction_type="epsilon",
                     thresholding=False, dynamic_thresholding_ratio=0.995, clip_sample_range=1.0,
                     sample_max_value=1.0, timestep_spacing="leading", steps_offset=0)
    _choices = dict(beta_schedule=("linear", "scaled_linear", "squaredcos_cap_v2"), trained_betas=(None,),
                    variance_type=("fixed_small",), prediction_type=("epsilon", "sample", "v_prediction"),
                    timestep_spacing=("leading", "linspace", "trailing"))
    _named_by_diffusers = ("prediction_type",)

    def _check_extra(self, cfg):
        self._check_thresholding(cfg)

    def set_timesteps(self, num_inference_steps: int, device=None):
        n_train = self.config.num_train_timesteps
        if num_inference_steps > n_train:
            raise ValueError(f"num_inference_steps {num_inference_steps} > num_train_timesteps {n_train}")
        self.num_inference_steps = num_inference_steps
        spacing = self.config.get("timestep_spacing", "leading")
        if spacing == "leading":
            ratio = n_train // num_inference_steps  # integer floor: 1000 // 750 == 1 (SURVEY headline finding 4)
            ts = (np.arange(0, num_inference_steps) * ratio).round()[::-1].copy().astype(np.int64)
            ts += self.config.steps_offset
        elif spacing == "linspace":
            ts = np.linspace(0, n_train - 1, num_inference_steps).round()[::-1].copy().astype(np.int64)
        else:       # "trailing": the table starts at the LAST training timestep (Lin et al., 2023, section 3.2)
            ts = (np.round(np.arange(n_train, 0, -n_train / num_inference_steps)) - 1).astype(np.int64)
        self.timesteps = torch.from_numpy(ts).to(device) if device is not None else torch.from_numpy(ts)

    def previous_timestep(self, t: int) -> int:
        n = self.num_inference_steps if self.num_inference_steps else self.config.num_train_timesteps
        return t - self.config.num_train_timesteps // n

    # ---- reverse step -----------------------------------------------------------------------------
    def step_scalars(self, t: int):
        """fp32 scalars of DDPMScheduler.step for timestep t, in the reference's operation order (memoised per
        (t, previous timestep))."""
        return self._memo(self._scalar_cache, (t, self.previous_timestep(t)), lambda: self._step_scalars(t))

    def _step_scalars(self, t: int):
        prev_t = self.previous_timestep(t)
        a_t = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.one
        b_t = 1 - a_t
        b_prev = 1 - a_prev
        cur_alpha = a_t / a_prev
        cur_beta = 1 - cur_alpha
        c0 = (a_prev ** 0.5 * cur_beta) / b_t
        ct = cur_alpha ** 0.5 * b_prev / b_t
        var = torch.clamp(b_prev / b_t * cur_beta, min=1e-20)
        return dict(sqrt_beta_prod_t=float(b_t ** 0.5), sqrt_alpha_prod_t=float(a_t ** 0.5), coef_x0=float(c0),
                    coef_xt=float(ct), sigma=float(var ** 0.5))

    @staticmethod
    def _check_pt_inputs(who, sample, model_output):
        if sample.dtype != torch.float32 or model_output.dtype != torch.float32:
            raise ValueError(f"{who}: fp32 only")
        if tuple(model_output.shape) != tuple(sample.shape):
            raise ValueError(f"{who}: model output {tuple(model_output.shape)} != sample {tuple(sample.shape)}")

    def step(self, model_output, timestep, sample, generator=None, return_dict: bool = True, variance_noise=None):
        if not sample.is_cuda:
            raise RuntimeError("DDPMScheduler.step runs on the MI355X HIP engine only (got a CPU tensor)")
        t = int(timestep)
        s = self.step_scalars(t)
        nz = _resolve_noise(variance_noise, sample, generator) if t > 0 else _StepNoise()    # (t == 0 has no noise term)
        x, e = sample.contiguous(), model_output.contiguous()
        prev = torch.empty_like(x)
        clip = self.config.clip_sample_range if self.config.clip_sample else 0.0
        with torch.cuda.device(x.device):
            if self.config.thresholding:        # (takes precedence over clip_sample, as in diffusers)
                self._check_thresholded_inputs("DDPMScheduler.step", x, e)
                scale, per = self._threshold_scale(x, e, s)
                _lib.check(_lib.load().dsg_ddpm_step_thr(_lib.ptr(x), _lib.ptr(e), nz.ptr, _lib.ptr(scale), _lib.ptr(prev),
                                                        x.numel(), per, s["sqrt_beta_prod_t"], s["sqrt_alpha_prod_t"],
                                                        s["coef_x0"], s["coef_xt"], s["sigma"], _lib.stream_ptr(x.device)))
            elif self.config.prediction_type == "epsilon":
                _lib.check(_lib.load().dsg_ddpm_step(_lib.ptr(x), _lib.ptr(e), nz.ptr, _lib.ptr(prev), x.numel(),
                                                    s["sqrt_beta_prod_t"], s["sqrt_alpha_prod_t"], clip, s["coef_x0"],
                                                    s["coef_xt"], s["sigma"], _lib.stream_ptr(x.device)))
            else:
                self._check_pt_inputs("DDPMScheduler.step", x, e)
                _lib.check(_lib.load().dsg_ddpm_step_pt(_lib.ptr(x), _lib.ptr(e), nz.ptr, _lib.ptr(prev), x.numel(),
                                                       _lib.PRED_CODES[self.config.prediction_type], s["sqrt_beta_prod_t"],
                                                       s["sqrt_alpha_prod_t"], clip, s["coef_x0"], s["coef_xt"], s["sigma"],
                                                       _lib.stream_ptr(x.device)))
            _record_consumed(nz, x.device)
        if not return_dict:
            return (prev,)
        return SchedulerOutput(prev_sample=prev)


class DDIMScheduler(DDPMScheduler):
    _class_name = "DDIMScheduler"
    _defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                     trained_betas=None, clip_sample=True, set_alpha_to_one=True, steps_offset=0,
                     prediction_type="epsilon", thresholding=False, dynamic_thresholding_ratio=0.995,
                     clip_sample_range=1.0, sample_max_value=1.0, timestep_spacing="leading",
                     rescale_betas_zero_snr=False)
    _choices = dict(beta_schedule=("linear", "scaled_linear", "squaredcos_cap_v2"), trained_betas=(None,),
                    prediction_type=("epsilon", "sample", "v_prediction"), timestep_spacing=("leading", "linspace", "trailing"),
                    rescale_betas_zero_snr=(False, True))

    def _check_extra(self, cfg):
        self._check_thresholding(cfg)
        if cfg["thresholding"] and cfg["rescale_betas_zero_snr"]:
            raise NotImplementedError("DDIMScheduler: rescale_betas_zero_snr=True with thresholding=True is outside the "
                                      "DriveSceneGen path (supported: False)")

    def _betas(self, cfg):
        betas = super()._betas(cfg)
        if not cfg.get("rescale_betas_zero_snr", False):
            return betas
        # diffusers' rescale_zero_terminal_snr (Lin et al., 2023, Algorithm 1) in fp32: shift sqrt(abar) so that its last entry
        # is exactly 0, scale so that its first entry is unchanged
        s = torch.cumprod(1.0 - betas, dim=0).sqrt()
        a0, aT = s[0].clone(), s[-1].clone()
        s -= aT
        s *= a0 / (a0 - aT)
        ab = s ** 2
        return 1 - torch.cat([ab[0:1], ab[1:] / ab[:-1]])

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        # (a subclass whose config has no such key -- RePaint -- ends at alpha-bar = 1, as diffusers' does)
        self.final_alpha_cumprod = torch.tensor(1.0) if self.config.get("set_alpha_to_one", True) else self.alphas_cumprod[0]

    def step_scalars(self, t: int, eta: float = 0.0):
        return self._memo(self._scalar_cache, (t, self.previous_timestep(t), float(eta)), lambda: self._step_scalars(t, eta))

    def _step_scalars(self, t: int, eta: float = 0.0):
        prev_t = self.previous_timestep(t)
        a_t = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
        b_t = 1 - a_t
        b_prev = 1 - a_prev
        variance = (b_prev / b_t) * (1 - a_t / a_prev)
        std = eta * variance ** 0.5
        dirc = (1 - a_prev - std ** 2) ** 0.5
        return dict(sqrt_beta_prod_t=float(b_t ** 0.5), sqrt_alpha_prod_t=float(a_t ** 0.5),
                    sqrt_alpha_prev=float(a_prev ** 0.5), dir_coef=float(dirc), std=float(std))

    def step(self, model_output, timestep, sample, eta: float = 0.0, use_clipped_model_output: bool = False,
             generator=None, variance_noise=None, return_dict: bool = True):
        if use_clipped_model_output:
            raise NotImplementedError("DDIMScheduler.step: use_clipped_model_output is outside the benchmarked path")
        if not sample.is_cuda:
            raise RuntimeError("DDIMScheduler.step runs on the MI355X HIP engine only (got a CPU tensor)")
        t = int(timestep)
        s = self.step_scalars(t, eta)
        x, e = sample.contiguous(), model_output.contiguous()
        prev = torch.empty_like(x)
        clip = self.config.clip_sample_range if self.config.clip_sample else 0.0
        with torch.cuda.device(x.device):
            if self.config.thresholding:        # (takes precedence over clip_sample, as in diffusers)
                self._check_thresholded_inputs("DDIMScheduler.step", x, e)
                scale, per = self._threshold_scale(x, e, s)
                _lib.check(_lib.load().dsg_ddim_step_thr(_lib.ptr(x), _lib.ptr(e), _lib.ptr(scale), _lib.ptr(prev), x.numel(),
                                                        per, s["sqrt_beta_prod_t"], s["sqrt_alpha_prod_t"],
                                                        s["sqrt_alpha_prev"], s["dir_coef"], _lib.stream_ptr(x.device)))
            elif self.config.prediction_type == "epsilon":
                _lib.check(_lib.load().dsg_ddim_step(_lib.ptr(x), _lib.ptr(e), _lib.ptr(prev), x.numel(),
                                                    s["sqrt_beta_prod_t"], s["sqrt_alpha_prod_t"], clip,
                                                    s["sqrt_alpha_prev"], s["dir_coef"], _lib.stream_ptr(x.device)))
            else:
                self._check_pt_inputs("DDIMScheduler.step", x, e)
                _lib.check(_lib.load().dsg_ddim_step_pt(_lib.ptr(x), _lib.ptr(e), _lib.ptr(prev), x.numel(),
                                                       _lib.PRED_CODES[self.config.prediction_type], s["sqrt_beta_prod_t"],
                                                       s["sqrt_alpha_prod_t"], clip, s["sqrt_alpha_prev"], s["dir_coef"],
                                                       _lib.stream_ptr(x.device)))
        if eta > 0:
            z = variance_noise if variance_noise is not None else _randn_like_reference(
                model_output.shape, generator, model_output.device, model_output.dtype)
            prev = prev + s["std"] * z.to(prev.device)
        if not return_dict:
            return (prev,)
        return SchedulerOutput(prev_sample=prev)


class _NoiseSource:
    """Where a scheduler's per-step noise comes from when the caller hands none in (``RePaintScheduler``,
    ``DPMSolverMultistepScheduler``; read by ``_resolve_noise``): the caller's generator (the default), or the Philox tensors
    (seed, offset), (seed, offset + 1), ... of ``dsg_philox_normal``, generated inside the step kernel -- the same distribution,
    not the same values."""

    noise_mode, noise_seed, noise_offset = "host", None, 0

    def use_host_noise(self):
        self.noise_mode, self.noise_seed, self.noise_offset = "host", None, 0

    def use_device_noise(self, seed: int, offset: int = 0):
        """Every later draw is the Philox4x32-10 / Box-Muller tensor (seed, offset), (seed, offset + 1), ... of
        ``dsg_philox_normal`` (same distribution as the host mode, not the same values)."""
        if seed is None:
            raise ValueError(f"{self._class_name}: noise='device' needs an integer seed")
        self.noise_mode, self.noise_seed, self.noise_offset = "device", int(seed) & (2 ** 64 - 1), int(offset)

    def _next_offset(self):
        k, self.noise_offset = self.noise_offset, self.noise_offset + 1
        return k & (2 ** 64 - 1)

    def device_randn(self, shape, device):
        """One device-mode draw as a tensor of its own (the pipeline's x_T): ``dsg_philox_normal`` at the next offset."""
        if self.noise_mode != "device":
            raise RuntimeError(f"{self._class_name}.device_randn: call use_device_noise(seed) first")
        out = torch.empty(tuple(shape), dtype=torch.float32, device=device)
        with torch.cuda.device(out.device):
            _lib.check(_lib.load().dsg_philox_normal(_lib.ptr(out), out.numel(), self.noise_seed, self._next_offset(),
                                                    _lib.stream_ptr(out.device)))
        return out


def _broadcast_extents(name, t, full, free):
    """`t` must be a 4-d tensor whose extents equal `full` except, on the axes listed in `free`, where 1 is allowed."""
    if t.dim() != 4 or any(int(t.shape[i]) != full[i] and not (i in free and int(t.shape[i]) == 1) for i in range(4)):
        allowed = "[" + ", ".join(f"{full[i]} or 1" if i in free else str(full[i]) for i in range(4)) + "]"
        raise ValueError(f"RePaintScheduler.step: {name} has shape {tuple(t.shape)}, expected {allowed}")


class RePaintScheduler(DDIMScheduler, _NoiseSource):
    """diffusers-0.20.0 ``RePaintScheduler`` (Lugmayr et al., "RePaint: Inpainting using Denoising Diffusion Probabilistic
    Models", CVPR 2022, Algorithm 1): the DDIM-form reverse step of an UNCONDITIONAL network with the known region replaced,
    at every step, by the original noised to that step's level, and ``undo_step`` -- the jump back in time that lets the
    generated part harmonise with the known part.  diffusers is not installed where this project builds and the reference
    tree holds no RePaint code: the formulas in include/dsg.h (``dsg_repaint_step``) and the paper are the specification.

    Host side: the jump schedule (``set_timesteps``) and the per-step fp32 scalars, the latter through
    ``DDIMScheduler._step_scalars``.  Device side: ONE ``dsg_repaint_step`` per reverse step, one ``dsg_repaint_undo`` per
    forward-diffusion pass.

    Noise.  By default every draw comes from the caller's generator in diffusers' order and shapes (one tensor per ``step``,
    ``num_train_timesteps // num_inference_steps`` per ``undo_step``; a CPU generator draws on the host), so a seeded call
    is reproducible against diffusers.  ``use_device_noise(seed)`` is this package's extension (like
    ``train_steps(noise="device")``): nothing is drawn on the host, draw k of the scheduler is the Philox tensor named
    (seed, offset + k) and is generated inside the step kernel, and ``undo_step`` is ONE pass with the closed form of its
    passes, ``ck = sqrt(prod(1 - beta_i))``, ``cz = sqrt(1 - prod(1 - beta_i))``: the same distribution as the host mode,
    NOT the same values."""

    _class_name = "RePaintScheduler"
    _defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", eta=0.0,
                     trained_betas=None, clip_sample=True)
    # (diffusers' RePaintScheduler has no thresholding keys: passing one is an unexpected argument, and its step never thresholds)
    _choices = dict(beta_schedule=("linear",), trained_betas=(None,))
    _named_by_diffusers = ()

    def _check_extra(self, cfg):
        pass

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.eta = float(self.config.eta)       # (diffusers: the pipeline overwrites this attribute per call)
        self._undo_cache = {}
        self.use_host_noise()

    # ---- timestep table ---------------------------------------------------------------------------------------
    def set_timesteps(self, num_inference_steps: int, jump_length: int = 10, jump_n_sample: int = 10, device=None):
        n_train = self.config.num_train_timesteps
        n = min(n_train, int(num_inference_steps))
        if n < 1 or jump_length < 1 or jump_n_sample < 1:
            raise ValueError("RePaintScheduler.set_timesteps: num_inference_steps, jump_length and jump_n_sample must be >= 1")
        self.num_inference_steps = n
        jumps = {j: jump_n_sample - 1 for j in range(0, n - jump_length, jump_length)}
        ts, t = [], n
        while t >= 1:
            t -= 1
            ts.append(t)
            if jumps.get(t, 0) > 0:
                jumps[t] -= 1
                for _ in range(jump_length):
                    t += 1
                    ts.append(t)
        ts = np.array(ts, dtype=np.int64) * (n_train // n)
        self.timesteps = torch.from_numpy(ts).to(device) if device is not None else torch.from_numpy(ts)

    # ---- scalars ----------------------------------------------------------------------------------------------
    def _step_scalars(self, t: int, eta: float = 0.0):
        s = super()._step_scalars(t, eta)
        prev_t = self.previous_timestep(t)
        a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
        s["sqrt_beta_prev"] = float((1 - a_prev) ** 0.5)
        return s

    def undo_scalars(self, t: int):
        """[(ck, cz)] of ``undo_step(sample, t)``'s passes (host mode), and the closed form of all of them (device mode)."""
        ratio = self.config.num_train_timesteps // self.num_inference_steps

        def make():
            if t < 0 or t + ratio > self.config.num_train_timesteps:
                raise ValueError(f"RePaintScheduler.undo_step: timestep {t} + {ratio} passes leaves the beta table")
            betas = [self.betas[t + i] for i in range(ratio)]
            passes = [(float((1 - b) ** 0.5), float(b ** 0.5)) for b in betas]
            keep = float(np.prod([1.0 - float(b) for b in betas], dtype=np.float64))
            return passes, (float(np.float32(np.sqrt(keep))), float(np.float32(np.sqrt(1.0 - keep))))
        return self._memo(self._undo_cache, (t, ratio), make)

    # ---- reverse step -----------------------------------------------------------------------------------------
    def step(self, model_output, timestep, sample, original_image, mask, generator=None, return_dict: bool = True,
             variance_noise=None):
        """x_{t-1} from x_t, the network's output, the known scene and the mask (1 keeps, 0 generates).
        `original_image` is [N or 1, C, H, W], `mask` [N or 1, C or 1, H, W] (fp32, broadcast by the kernel).
        `variance_noise` (this package's extension, as in ``DDPMScheduler.step``): the call's noise tensor, already drawn --
        a device tensor or a ``HostNoise``; otherwise it is drawn here from `generator`, or named by (seed, offset) in
        device-noise mode."""
        if not sample.is_cuda:
            raise RuntimeError("RePaintScheduler.step runs on the MI355X HIP engine only (got a CPU tensor)")
        if sample.dim() != 4 or sample.dtype != torch.float32:
            raise ValueError("RePaintScheduler.step: the sample must be an fp32 [N, C, H, W] tensor")
        if tuple(model_output.shape) != tuple(sample.shape):
            raise ValueError(f"RePaintScheduler.step: model output {tuple(model_output.shape)} != sample {tuple(sample.shape)}")
        full = tuple(int(v) for v in sample.shape)
        _broadcast_extents("original_image", original_image, full, (0,))
        _broadcast_extents("mask", mask, full, (0, 1))
        t = int(timestep)
        s = self.step_scalars(t, self.eta)
        x, e = sample.contiguous(), model_output.contiguous()
        orig = original_image.to(x.device, torch.float32).contiguous()
        m = mask.to(x.device, torch.float32).contiguous()
        nz = _resolve_noise(variance_noise, x, generator, self)
        prev = torch.empty_like(x)
        a = _lib.RepaintStepArgs(
            sample=_lib.ptr(x), eps=_lib.ptr(e), original=_lib.ptr(orig), mask=_lib.ptr(m), noise=nz.ptr, prev=_lib.ptr(prev),
            noise_out=None, n=full[0], c=full[1], h=full[2], w=full[3], original_n=int(orig.shape[0]),
            mask_n=int(m.shape[0]), mask_c=int(m.shape[1]), add_std=int(t > 0 and self.eta > 0),
            sqrt_beta_prod_t=s["sqrt_beta_prod_t"], sqrt_alpha_prod_t=s["sqrt_alpha_prod_t"],
            clip=1.0 if self.config.clip_sample else 0.0, sqrt_alpha_prev=s["sqrt_alpha_prev"], dir_coef=s["dir_coef"],
            std=s["std"], sqrt_beta_prev=s["sqrt_beta_prev"], seed=nz.seed, offset=nz.offset)
        import ctypes
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().dsg_repaint_step(ctypes.byref(a), _lib.stream_ptr(x.device)))
            _record_consumed(nz, x.device)
        if not return_dict:
            return (prev,)
        return SchedulerOutput(prev_sample=prev)

    def undo_step(self, sample, timestep, generator=None, variance_noise=None):
        """Jump back: ``num_train_timesteps // num_inference_steps`` forward-diffusion passes from `timestep`, pass i with
        ``beta = betas[timestep + i]`` and a fresh noise tensor (diffusers' indexing and order of draws).  In device-noise
        mode: one pass with the closed form of all of them (class docstring).  `variance_noise`: the passes' noise tensors,
        already drawn (a sequence of device tensors / ``HostNoise``), or a callable returning the next one."""
        if not sample.is_cuda:
            raise RuntimeError("RePaintScheduler.undo_step runs on the MI355X HIP engine only (got a CPU tensor)")
        if sample.dtype != torch.float32:
            raise ValueError("RePaintScheduler.undo_step: fp32 only")
        passes, fused = self.undo_scalars(int(timestep))
        x = sample.contiguous()
        lib, st = _lib.load(), _lib.stream_ptr(x.device)
        with torch.cuda.device(x.device):
            # device mode with nothing handed in: the closed form is ONE pass, its noise the scheduler's next Philox tensor
            one_pass = self.noise_mode == "device" and variance_noise is None
            for i, (ck, cz) in enumerate([fused] if one_pass else passes):
                z = None if variance_noise is None else variance_noise() if callable(variance_noise) else variance_noise[i]
                nz = _resolve_noise(z, x, generator, self)
                out = torch.empty_like(x)
                _lib.check(lib.dsg_repaint_undo(_lib.ptr(x), nz.ptr, _lib.ptr(out), x.numel(), ck, cz, nz.seed, nz.offset, st))
                _record_consumed(nz, x.device)
                x = out
        return x


class DPMSolverMultistepScheduler(_SchedulerBase, _NoiseSource):
    """diffusers-0.20.0 ``DPMSolverMultistepScheduler`` (Lu et al., "DPM-Solver++: Fast Solver for Guided Sampling of Diffusion
    Probabilistic Models", 2022) in its data-prediction forms: ``algorithm_type`` "dpmsolver++" (the multistep exponential
    integrator of the diffusion ODE, orders 1-3; order 1 is DDIM) and "sde-dpmsolver++" (orders 1-2, one noise tensor per
    step).  One network call per step, like DDIM, at a higher order of accuracy in the step size: the sampler a diffusers
    user swaps in to cut the step count, ``pipe.scheduler = DPMSolverMultistepScheduler.from_config(pipe.scheduler.config)``.
    diffusers is not installed where this project builds and the reference tree holds no DPM-Solver code: include/dsg.h
    (``dsg_dpmsolver_step``), the paper and tests/dpmsolver_oracle.py are the specification.

    Host side: the timestep table, the order bookkeeping and the per-step fp32 scalars (0-d fp32 torch arithmetic, memoised).
    Device side: ONE ``dsg_dpmsolver_step`` per step -- it makes the data prediction, stores it as the newest history entry
    and consumes it in the same pass.  The history is a ring of ``solver_order`` device buffers: the entry that falls out of
    the history is the one the kernel writes, so no output aliases an input.

    Noise (SDE variant only), as in ``RePaintScheduler``: by default drawn from the caller's generator in diffusers' order
    and shape, or handed in as ``variance_noise`` (a device tensor or a ``HostNoise``); after ``use_device_noise(seed)`` draw k
    is the Philox tensor (seed, offset + k), generated inside the step kernel.

    Not built (raising): Karras sigmas, dynamic thresholding, the noise-prediction forms "dpmsolver" / "sde-dpmsolver",
    v-prediction, learned variances.  ``from_config`` of a DDPM / DDIM config with ``thresholding=True`` (or another ratio or
    maximum) therefore raises too; ``dsg_dynthresh_scale`` already takes this solver's (sigma_s, alpha_s).  ``variance_type`` "fixed_small" / "fixed_large" (what a converted DDPM config carries) are
    accepted: as in diffusers, only the learned forms would change this scheduler's arithmetic."""

    _class_name = "DPMSolverMultistepScheduler"
    _defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                     solver_order=2, prediction_type="epsilon", thresholding=False, dynamic_thresholding_ratio=0.995,
                     sample_max_value=1.0, algorithm_type="dpmsolver++", solver_type="midpoint", lower_order_final=True,
                     use_karras_sigmas=False, lambda_min_clipped=-float("inf"), variance_type=None,
                     timestep_spacing="linspace", steps_offset=0)
    _choices = dict(beta_schedule=("linear",), trained_betas=(None,), prediction_type=("epsilon",), thresholding=(False,),
                    dynamic_thresholding_ratio=(0.995,), sample_max_value=(1.0,), use_karras_sigmas=(False,),
                    lambda_min_clipped=(-float("inf"),), solver_order=(1, 2, 3), algorithm_type=("dpmsolver++", "sde-dpmsolver++"), solver_type=("midpoint", "heun"),
                    lower_order_final=(True, False), timestep_spacing=("linspace", "leading", "trailing"),
                    variance_type=(None, "fixed_small", "fixed_large"))

    def _check_extra(self, cfg):
        if isinstance(cfg["steps_offset"], bool) or not isinstance(cfg["steps_offset"], (int, np.integer)):
            raise NotImplementedError(f"{self._class_name}: steps_offset={cfg['steps_offset']!r} is outside the DriveSceneGen "
                                      "path (supported: an integer)")
        if cfg["algorithm_type"] == "sde-dpmsolver++" and cfg["solver_order"] == 3:
            raise NotImplementedError(f"{self._class_name}: algorithm_type='sde-dpmsolver++' has orders 1 and 2 only "
                                      "(solver_order=3 is outside the DriveSceneGen path)")

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.alpha_t = torch.sqrt(self.alphas_cumprod)
        self.sigma_t = torch.sqrt(1 - self.alphas_cumprod)
        self.lambda_t = torch.log(self.alpha_t) - torch.log(self.sigma_t)
        self.timesteps = torch.from_numpy(np.linspace(0, self.config.num_train_timesteps - 1, self.config.num_train_timesteps,
                                                      dtype=np.float32)[::-1].copy().astype(np.int64))
        self.lower_order_nums = 0
        self._hist_t = []                       # timesteps of the history entries, newest first
        self._ring, self._head = None, 0        # solver_order device buffers; _ring[_head] holds the newest entry
        self._index = None
        self.use_host_noise()

    @property
    def needs_step_noise(self):
        """Does ``step`` consume one noise tensor per call?  (what a pipeline's noise stream has to count)"""
        return self.config.algorithm_type == "sde-dpmsolver++"

    # ---- timestep table ---------------------------------------------------------------------------------------
    def set_timesteps(self, num_inference_steps: int, device=None):
        n_train, n = self.config.num_train_timesteps, int(num_inference_steps)
        if n < 1 or n > n_train:
            raise ValueError(f"num_inference_steps {num_inference_steps} outside [1, num_train_timesteps {n_train}]")
        spacing = self.config.timestep_spacing
        if spacing == "linspace":
            ts = np.linspace(0, n_train - 1, n + 1).round()[::-1][:-1]
        elif spacing == "leading":
            ts = (np.arange(0, n + 1) * (n_train // (n + 1))).round()[::-1][:-1] + self.config.steps_offset
        else:
            ts = np.arange(n_train, 0, -n_train / n).round() - 1
        ts = ts.copy().astype(np.int64)
        _, first = np.unique(ts, return_index=True)          # drop duplicates, keep the order
        ts = ts[np.sort(first)]
        if ts.min() < 0 or ts.max() >= n_train:
            raise ValueError(f"{self._class_name}: steps_offset={self.config.steps_offset} puts a timestep outside "
                             f"[0, {n_train - 1}]")
        self.timesteps = torch.from_numpy(ts).to(device) if device is not None else torch.from_numpy(ts)
        self.num_inference_steps = len(ts)
        self._index = {int(t): i for i, t in enumerate(ts)}
        self._hist_t, self.lower_order_nums = [], 0

    # ---- order bookkeeping and scalars ----------------------------------------------------------------------------
    def _order_at(self, i: int) -> int:
        """The order the step at index `i` of the table uses, given ``lower_order_nums`` history entries so far."""
        so, L = self.config.solver_order, len(self.timesteps)
        short = self.config.lower_order_final and L < 15
        if so == 1 or self.lower_order_nums < 1 or (i == L - 1 and short):
            return 1
        if so == 2 or self.lower_order_nums < 2 or (i == L - 2 and short):
            return 2
        return 3

    def step_scalars(self, s0: int, t: int, s1=None, s2=None, order: int = 1):
        """The fp32 scalars ``dsg_dpmsolver_step`` takes for the step s0 -> t that uses `order`, with the history entries made
        at s1 and s2 (memoised: some twenty 0-d tensor operations otherwise)."""
        key = (s0, t, s1 if order >= 2 else None, s2 if order >= 3 else None, order, self.config.algorithm_type,
               self.config.solver_type)
        return self._memo(self._scalar_cache, key, lambda: self._step_scalars(s0, t, s1, s2, order))

    def _step_scalars(self, s0, t, s1, s2, order):
        lam, al, sg = self.lambda_t, self.alpha_t, self.sigma_t
        sde = self.config.algorithm_type == "sde-dpmsolver++"
        heun = self.config.solver_type == "heun"
        alpha_t, sigma_t, sigma_s0 = al[t], sg[t], sg[s0]
        h = lam[t] - lam[s0]
        out = dict(sigma_s=sigma_s0, alpha_s=al[s0], inv_r0=0.0, inv_r1=0.0, q=0.0, p=0.0, c1=0.0, c2=0.0, cn=0.0)
        if order >= 2:
            h0 = lam[s0] - lam[s1]
            r0 = h0 / h
            out["inv_r0"] = 1.0 / r0
        if order == 3:
            h1 = lam[s1] - lam[s2]
            r1 = h1 / h
            out["inv_r1"] = 1.0 / r1
            out["q"] = r0 / (r0 + r1)
            out["p"] = 1.0 / (r0 + r1)
        if not sde:
            E = torch.exp(-h) - 1.0
            out["kx"] = sigma_t / sigma_s0
            out["c0"] = -(alpha_t * E)
            if order == 2 and not heun:
                out["c1"] = -(0.5 * (alpha_t * E))
            elif order >= 2:
                out["c1"] = alpha_t * (E / h + 1.0)
            if order == 3:
                out["c2"] = -(alpha_t * ((E + h) / h ** 2 - 0.5))
        else:
            G = 1.0 - torch.exp(-2.0 * h)
            out["kx"] = sigma_t / sigma_s0 * torch.exp(-h)
            out["c0"] = alpha_t * G
            if order == 2:
                out["c1"] = alpha_t * (G / (-2.0 * h) + 1.0) if heun else 0.5 * (alpha_t * G)
            out["cn"] = sigma_t * torch.sqrt(G)
        return {k: float(v) for k, v in out.items()}

    # ---- the step ---------------------------------------------------------------------------------------------
    def _history(self, like):
        """The ring of ``solver_order`` history buffers for samples like `like` (allocated on first use, and again when the
        shape or the device changes -- which is only legal at the start of a run)."""
        r = self._ring
        if r is None or r[0].shape != like.shape or r[0].device != like.device:
            if self.lower_order_nums > 0:
                raise ValueError(f"{self._class_name}.step: the sample changed shape or device in the middle of a run "
                                 "(call set_timesteps to start another)")
            self._ring = [torch.empty_like(like) for _ in range(self.config.solver_order)]
            self._head = 0
        return self._ring

    def step(self, model_output, timestep, sample, generator=None, variance_noise=None, return_dict: bool = True):
        if not sample.is_cuda:
            raise RuntimeError(f"{self._class_name}.step runs on the MI355X HIP engine only (got a CPU tensor)")
        if sample.dtype != torch.float32 or model_output.dtype != torch.float32:
            raise ValueError(f"{self._class_name}.step: fp32 only")
        if tuple(model_output.shape) != tuple(sample.shape):
            raise ValueError(f"{self._class_name}.step: model output {tuple(model_output.shape)} != sample {tuple(sample.shape)}")
        if self._index is None:
            raise ValueError(f"{self._class_name}.step: call set_timesteps first")
        ts = self.timesteps
        L = len(ts)
        s0 = int(timestep)
        i = self._index.get(s0, L - 1)          # (diffusers: a timestep the table lacks is taken for the last one)
        t = int(ts[i + 1]) if i + 1 < L else 0
        order = self._order_at(i)
        s1 = self._hist_t[0] if order >= 2 else None
        s2 = self._hist_t[1] if order >= 3 else None
        s = self.step_scalars(s0, t, s1, s2, order)
        x, e = sample.contiguous(), model_output.contiguous()
        ring = self._history(x)
        K = len(ring)
        m1 = ring[self._head] if order >= 2 else None
        m2 = ring[(self._head - 1) % K] if order >= 3 else None
        slot = (self._head + 1) % K if self._hist_t else self._head     # the entry that falls out of the history
        sde = self.needs_step_noise
        nz = _resolve_noise(variance_noise, x, generator, self) if sde else _StepNoise()
        prev = torch.empty_like(x)
        a = _lib.DpmSolverStepArgs(
            sample=_lib.ptr(x), eps=_lib.ptr(e), m1=_lib.ptr(m1), m2=_lib.ptr(m2), noise=nz.ptr, prev=_lib.ptr(prev),
            m0_out=_lib.ptr(ring[slot]), noise_out=None, numel=x.numel(), order=order, add_noise=int(sde),
            sigma_s=s["sigma_s"], alpha_s=s["alpha_s"], inv_r0=s["inv_r0"], inv_r1=s["inv_r1"], q=s["q"], p=s["p"],
            kx=s["kx"], c0=s["c0"], c1=s["c1"], c2=s["c2"], cn=s["cn"], seed=nz.seed, offset=nz.offset)
        import ctypes
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().dsg_dpmsolver_step(ctypes.byref(a), _lib.stream_ptr(x.device)))
            _record_consumed(nz, x.device)
        self._head = slot
        self._hist_t = ([s0] + self._hist_t)[:K]
        if self.lower_order_nums < self.config.solver_order:
            self.lower_order_nums += 1
        if not return_dict:
            return (prev,)
        return SchedulerOutput(prev_sample=prev)
