"""``DDPMPipeline`` / ``DDIMPipeline`` -- the sampler objects DriveSceneGen's scripts call -- and ``RePaintPipeline``, scene
completion (keep part of a scene, generate the rest) with the same unconditional network.

Reference call sites:
 - /root/reference/DriveSceneGen/pipeline/training_pipeline.py:101 ``DDPMPipeline(unet=..., scheduler=...)``,
   :26-32 ``pipeline(num_inference_steps=750, batch_size, generator=torch.manual_seed(seed),
   output_type="np.array", return_dict=False)``, :107 ``pipeline.save_pretrained(output_dir)``;
 - /root/reference/DriveSceneGen/scripts/generation.py:7 ``DDPMPipeline.from_pretrained(path, variant="fp16")
   .to('cuda')`` and :14-20 ``ddpm(batch_size=5, num_inference_steps=750).images``.
Semantics: SURVEY.md App. A.4 (noise stream order, post-processing) and A.5 (folder layout).

The denoising loop stays host-driven like the reference's, but each iteration is two asynchronous C-ABI
calls on the current HIP stream (dsg_unet_forward + dsg_ddpm_step / dsg_ddim_step); batched inference
shards samples over ranks with no collective (``shard=(rank, world)``).
"""
from __future__ import annotations

import json
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from .schedulers import DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler, RePaintScheduler, _randn_like_reference
from .unet import UNet2DModel


class ImagePipelineOutput(SimpleNamespace):
    pass


def numpy_to_pil(images: np.ndarray):
    """diffusers ``numpy_to_pil``: (x*255).round().astype(uint8); C=1 -> mode L."""
    from PIL import Image
    if images.ndim == 3:
        images = images[None, ...]
    images = (images * 255).round().astype("uint8")
    if images.shape[-1] == 1:
        return [Image.fromarray(im.squeeze(), mode="L") for im in images]
    if images.shape[-1] not in (3, 4):
        raise ValueError(f"PIL output supports 1, 3 or 4 channels (got {images.shape[-1]}); "
                         "use output_type='np.array'")
    return [Image.fromarray(im) for im in images]


class _PipelineBase:
    _class_name = "DDPMPipeline"
    _scheduler_cls = DDPMScheduler
    _kept_scheduler_classes = ()    # scheduler classes a saved folder may name that this pipeline runs as they are

    def __init__(self, unet, scheduler):
        self.unet = unet
        self.scheduler = scheduler

    @property
    def device(self):
        return self.unet.device

    def to(self, device):
        self.unet.to(device)
        return self

    # ---- App. A.5 folder layout -------------------------------------------------------------------
    def save_pretrained(self, save_directory, safe_serialization: bool = False, variant=None):
        os.makedirs(save_directory, exist_ok=True)
        index = {"_class_name": self._class_name, "_diffusers_version": "0.20.0",
                 "scheduler": ["diffusers", type(self.scheduler)._class_name],
                 "unet": ["diffusers", "UNet2DModel"]}
        with open(os.path.join(save_directory, "model_index.json"), "w") as f:
            json.dump(index, f, indent=2, sort_keys=True)
            f.write("\n")
        self.unet.save_pretrained(os.path.join(save_directory, "unet"), safe_serialization=safe_serialization,
                                  variant=variant)
        self.scheduler.save_pretrained(os.path.join(save_directory, "scheduler"))

    @classmethod
    def from_pretrained(cls, path, variant=None, torch_dtype=None, **_unused):
        with open(os.path.join(path, "model_index.json")) as f:
            index = json.load(f)
        sched_name = index.get("scheduler", ["diffusers", "DDPMScheduler"])[1]
        sched_cls = {"DDPMScheduler": DDPMScheduler, "DDIMScheduler": DDIMScheduler,
                     "RePaintScheduler": RePaintScheduler,
                     "DPMSolverMultistepScheduler": DPMSolverMultistepScheduler}.get(sched_name)
        if sched_cls is None:
            raise NotImplementedError(f"scheduler class {sched_name!r} not supported")
        if cls._scheduler_cls is not sched_cls and sched_cls not in cls._kept_scheduler_classes:
            # diffusers lets a pipeline adopt a compatible scheduler config
            scheduler = cls._scheduler_cls.from_config(
                {k: v for k, v in json.load(open(os.path.join(path, "scheduler", "scheduler_config.json"))).items()})
        else:
            scheduler = sched_cls.from_pretrained(path, subfolder="scheduler")
        unet = UNet2DModel.from_pretrained(path, subfolder="unet", variant=variant, torch_dtype=torch_dtype)
        return cls(unet=unet, scheduler=scheduler)

    # ---- shared loop --------------------------------------------------------------------------------
    def _initial_noise(self, batch_size, generator, shard):
        c = self.unet.config
        ss = c.sample_size
        shape = (batch_size, c.in_channels, ss, ss) if isinstance(ss, int) else (batch_size, c.in_channels, *ss)
        image = _randn_like_reference(shape, generator, self.device, torch.float32)
        return self._shard(image, shard)

    @staticmethod
    def _shard(x, shard):
        if shard is None:
            return x
        rank, world = shard
        b = x.shape[0]
        if b % world != 0:
            raise ValueError(f"batch {b} not divisible by world size {world}")
        per = b // world
        return x[rank * per:(rank + 1) * per].contiguous()

    def _finish(self, image, output_type, return_dict):
        b, c, h, w = image.shape
        out = torch.empty((b, h, w, c), dtype=torch.float32, device=image.device)
        with torch.cuda.device(image.device):
            _lib.check(_lib.load().dsg_postprocess(_lib.ptr(image.contiguous()), _lib.ptr(out), b, c, h * w, 0,
                                                  _lib.stream_ptr(image.device)))
        arr = out.cpu().numpy()
        if output_type == "pil":
            arr = numpy_to_pil(arr)
        if not return_dict:
            return (arr,)
        return ImagePipelineOutput(images=arr)


class _NoiseStream:
    """The per-step noise of ``DDPMPipeline.__call__`` in the reference's order of draws (App. A.4: x_T, then one full-batch
    tensor per step with t > 0, all from ONE generator).  A CPU generator (training_pipeline.py:29 passes
    ``torch.manual_seed(seed)``) samples on the host: tensor k+1 is drawn by a worker thread into one of THREE pinned buffers while
    the caller enqueues step k's kernels, and the scheduler's step kernel reads that buffer in place, over PCIe
    (``schedulers.HostNoise``: the noise is read exactly once, 12 bytes per pixel of a batch-1 sample) -- same generator, same
    shapes, same order, so the same values as ``randn_tensor(...).to(device)`` bit for bit, with neither the draw, nor a
    pageable copy, nor a second stream's hand-over on the critical path.  Measured on the evaluate call (750 steps, batch 1;
    tools/whole_call_probe.py): device-RNG loop 2.15 ms per step; this 2.18; a pinned copy on the same stream 2.20; a copy on
    a side stream with event hand-overs 2.27.  `count` = the draws the call will make: the worker never draws past it, and
    ``close()`` (always called) joins it and, should the loop have ended early, puts the generator back where the serial
    loop would have left it.  With no generator, or a device generator, a draw is torch's device RNG kernel on the current
    stream, as in the reference."""

    RING = 3

    def __init__(self, shape, generator, device, rows=None, count=1):
        self.shape, self.gen, self.dev, self.rows, self.count = tuple(shape), generator, torch.device(device), rows, int(count)
        self.host = generator is not None and generator.device.type == "cpu"
        self.k = 0
        self._pending = None          # (thread, index, generator state before the draw, [exception])
        if self.host:
            # three buffers: the draw of tensor k waits for the kernel that read tensor k - 3, so the host may run two whole
            # steps ahead of the GPU (with two it stalled on the step before last: never more than one forward queued)
            self.pinned = [torch.empty(self.shape, dtype=torch.float32).pin_memory() for _ in range(self.RING)]
            self.lent = [None] * self.RING  # the HostNoise last handed out on pinned[i] (its `consumed` event guards the reuse)

    def _start(self, k):
        """hand tensor k's draw to a worker thread (one in flight at most; nobody else touches the generator meanwhile)"""
        import threading
        i = k % self.RING
        if self.lent[i] is not None:
            self.lent[i].wait_consumed()      # the step kernel that read pinned[i] three draws ago has run
            self.lent[i] = None
        box = []

        def work():
            try:
                torch.randn(self.shape, generator=self.gen, out=self.pinned[i])
            except BaseException as e:   # surfaced by draw()
                box.append(e)
        snap = self.gen.get_state()
        th = threading.Thread(target=work, daemon=True)
        th.start()
        self._pending = (th, k, snap, box)

    def close(self):
        if self._pending is not None:     # a tensor was drawn ahead and never asked for: undo the draw
            th, _, snap, _ = self._pending
            th.join()
            self.gen.set_state(snap)
            self._pending = None
        if self.host:
            for h in self.lent:           # the pinned buffers must outlive the kernels that read them
                if h is not None:
                    h.wait_consumed()
            self.lent = [None] * self.RING

    def draw(self):
        """The next tensor of the stream (this shard's rows of it): a device tensor, or -- host generator, after x_T -- a
        ``HostNoise`` over a pinned buffer, to be handed to ``scheduler.step(..., variance_noise=...)`` before the draw after
        next."""
        from .schedulers import HostNoise
        rows = self.rows
        k, self.k = self.k, self.k + 1
        if not self.host:
            z = torch.randn(self.shape, generator=self.gen, device=self.dev, dtype=torch.float32)
            return z if rows is None else z[rows].contiguous()
        if k == 0:   # x_T is the U-Net's first input: a device tensor, the reference's plain path
            z = torch.randn(self.shape, generator=self.gen, dtype=torch.float32)
            out = (z if rows is None else z[rows]).to(self.dev)
            if self.count > 1:
                self._start(1)
            return out
        i = k % self.RING
        if self._pending is None:             # (more draws than announced: drawn here, in order)
            self._start(k)
        th, kk, _, box = self._pending
        th.join()
        self._pending = None
        if box:
            raise box[0]
        assert kk == k
        out = HostNoise(self.pinned[i] if rows is None else self.pinned[i][rows])
        self.lent[i] = out
        if k + 1 < self.count:
            self._start(k + 1)                # drawn while the caller enqueues the rest of this step and the next forward
        return out


def _rows_of(shard, batch):
    if shard is None:
        return None
    rank, world = shard
    if batch % world != 0:
        raise ValueError(f"batch {batch} not divisible by world size {world}")
    per = batch // world
    return slice(rank * per, (rank + 1) * per)


def _device_timestep_rows(timesteps, batch, device):
    """[steps, batch] int64 on the device, uploaded ONCE per call: row i is the timestep tensor of step i (the loop then
    hands the U-Net a device view instead of a host scalar -- no H2D copy and no expand kernel per step)."""
    return timesteps.to(device=device, dtype=torch.long)[:, None].expand(-1, batch).contiguous()


def _is_dpmsolver(scheduler):
    return isinstance(scheduler, DPMSolverMultistepScheduler)


class DDPMPipeline(_PipelineBase):
    _class_name = "DDPMPipeline"
    _scheduler_cls = DDPMScheduler
    _kept_scheduler_classes = (DPMSolverMultistepScheduler,)

    @torch.no_grad()
    def __call__(self, batch_size: int = 1, generator=None, num_inference_steps: int = 1000, output_type="pil",
                 return_dict: bool = True, shard=None):
        if self.device.type != "cuda":
            raise RuntimeError("DDPMPipeline runs on the MI355X HIP engine only: call .to('cuda') first")
        c = self.unet.config
        ss = c.sample_size
        full = (batch_size, c.in_channels, ss, ss) if isinstance(ss, int) else (batch_size, c.in_channels, *ss)
        rows = _rows_of(shard, batch_size)
        with torch.cuda.device(self.device):
            # reference semantics: one generator stream for the whole batch (App. A.4); a shard draws the full-batch
            # tensors and keeps its rows so that N-GPU output == 1-GPU output
            self.scheduler.set_timesteps(num_inference_steps)
            ts = [int(t) for t in self.scheduler.timesteps]
            if _is_dpmsolver(self.scheduler):
                # the ODE solver takes no noise at all; its SDE variant one tensor per step, the last included -- from this
                # stream, unless the scheduler makes its own in the step kernel (use_device_noise)
                sch = self.scheduler
                if sch.needs_step_noise and sch.noise_mode == "device" and shard is not None:
                    raise NotImplementedError("DDPMPipeline: shard= with the SDE solver's device noise (every rank would "
                                              "generate the same tensor for different rows)")
                draws = [sch.needs_step_noise and sch.noise_mode != "device"] * len(ts)
            else:
                draws = [t > 0 for t in ts]
            stream = _NoiseStream(full, generator, self.device, rows, count=1 + sum(draws))
            try:
                image = stream.draw()
                tdev = _device_timestep_rows(self.scheduler.timesteps, image.shape[0], self.device)
                for i, t in enumerate(ts):
                    eps = self.unet(image, tdev[i]).sample
                    noise = stream.draw() if draws[i] else None  # (drawn while the previous step was enqueued; PCIe under the forward)
                    image = self.scheduler.step(eps, t, image, variance_noise=noise).prev_sample
            finally:
                stream.close()
        return self._finish(image, output_type, return_dict)


class DDIMPipeline(_PipelineBase):
    _class_name = "DDIMPipeline"
    _scheduler_cls = DDIMScheduler
    _kept_scheduler_classes = (DPMSolverMultistepScheduler,)

    @torch.no_grad()
    def __call__(self, batch_size: int = 1, generator=None, eta: float = 0.0, num_inference_steps: int = 50,
                 use_clipped_model_output=None, output_type="pil", return_dict: bool = True, shard=None):
        if self.device.type != "cuda":
            raise RuntimeError("DDIMPipeline runs on the MI355X HIP engine only: call .to('cuda') first")
        dpm = _is_dpmsolver(self.scheduler)
        if dpm and shard is not None and self.scheduler.needs_step_noise and self.scheduler.noise_mode == "device":
            raise NotImplementedError("DDIMPipeline: shard= with the SDE solver's device noise (every rank would generate "
                                      "the same tensor for different rows)")
        image = self._initial_noise(batch_size, generator, shard)
        self.scheduler.set_timesteps(num_inference_steps)
        ts = [int(t) for t in self.scheduler.timesteps]
        tdev = _device_timestep_rows(self.scheduler.timesteps, image.shape[0], self.device)
        for i, t in enumerate(ts):
            eps = self.unet(image, tdev[i]).sample
            if dpm:     # (no eta in its signature; its SDE variant draws each step's noise from `generator`, as eta > 0 does)
                image = self.scheduler.step(eps, t, image, generator=generator).prev_sample
            else:
                image = self.scheduler.step(eps, t, image, eta=eta, generator=generator).prev_sample
        return self._finish(image, output_type, return_dict)


def _is_pil(x):
    try:
        from PIL import Image
    except ImportError:
        return False
    return isinstance(x, Image.Image)


def _as_model_domain(image):
    """`image` -> float32 host tensor [N, C, H, W] in the model's domain: float tensors / arrays are taken as they are
    ([N, C, H, W] or [C, H, W]); PIL images and uint8 arrays ([.., H, W, C] or [H, W]) are mapped by x/255*2 - 1 (diffusers'
    ``_preprocess_image`` without its resize)."""
    if isinstance(image, (list, tuple)):
        if not image:
            raise ValueError("RePaintPipeline: empty image list")
        return torch.cat([_as_model_domain(im) for im in image], dim=0)
    if _is_pil(image):
        image = np.array(image)
        if image.dtype != np.uint8:
            raise ValueError(f"RePaintPipeline: PIL image of mode with dtype {image.dtype} not supported (8-bit modes only)")
    if isinstance(image, torch.Tensor):
        if image.dtype == torch.uint8:
            image = image.cpu().numpy()
        else:
            t = image.detach().to("cpu", torch.float32)
            if t.dim() == 3:
                t = t[None]
            if t.dim() != 4:
                raise ValueError(f"RePaintPipeline: image must be [N, C, H, W] (got shape {tuple(image.shape)})")
            return t.contiguous()
    arr = np.asarray(image)
    if arr.dtype == np.uint8:
        if arr.ndim == 2:
            arr = arr[..., None]
        if arr.ndim == 3:
            arr = arr[None]
        if arr.ndim != 4:
            raise ValueError(f"RePaintPipeline: uint8 image must be [N, H, W, C] (got shape {arr.shape})")
        arr = arr.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255.0) * np.float32(2.0) - np.float32(1.0)
        return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32))
    if not np.issubdtype(arr.dtype, np.floating):
        raise ValueError(f"RePaintPipeline: image dtype {arr.dtype} not supported (float in the model's domain, or uint8)")
    return _as_model_domain(torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32)))


def _as_binary_mask(mask):
    """`mask` -> float32 host tensor [N, C, H, W] of 0 / 1 (< 0.5 -> 0, else 1; 1 keeps): float / bool tensors and arrays
    [N, C, H, W], [C, H, W] or [H, W]; PIL "L" images and uint8 arrays are scaled by 1/255 first."""
    if isinstance(mask, (list, tuple)):
        if not mask:
            raise ValueError("RePaintPipeline: empty mask list")
        return torch.cat([_as_binary_mask(m) for m in mask], dim=0)
    if _is_pil(mask):
        mask = np.array(mask.convert("L"))
    if isinstance(mask, torch.Tensor):
        mask = mask.detach().cpu().numpy()
    arr = np.asarray(mask)
    if arr.dtype == np.uint8:
        arr = arr.astype(np.float32) / np.float32(255.0)
    elif arr.dtype == np.bool_ or np.issubdtype(arr.dtype, np.floating):
        arr = arr.astype(np.float32)
    else:
        raise ValueError(f"RePaintPipeline: mask dtype {arr.dtype} not supported (float, bool or uint8)")
    if arr.ndim == 2:
        arr = arr[None, None]
    elif arr.ndim == 3:
        arr = arr[None]
    if arr.ndim != 4:
        raise ValueError(f"RePaintPipeline: mask_image must be [N, C, H, W] (got shape {arr.shape})")
    return torch.from_numpy(np.ascontiguousarray((arr >= 0.5).astype(np.float32)))


class RePaintPipeline(_PipelineBase):
    """Scene completion (diffusers 0.20.0 ``RePaintPipeline``; Lugmayr et al., CVPR 2022): where ``mask_image`` is 1 the
    result IS ``image``; where it is 0 the unconditional network generates content that agrees with the kept part.  The mask
    may differ per channel (keep the lane planes of a raster, re-draw the agent plane).  Each entry of the jump schedule is
    either a U-Net forward + ONE ``dsg_repaint_step``, or a ``dsg_repaint_undo`` (the jump back in time)."""

    _class_name = "RePaintPipeline"
    _scheduler_cls = RePaintScheduler

    def _check_inputs(self, image, mask_image, batch_size):
        c = self.unet.config
        ss = c.sample_size
        h, w = (ss, ss) if isinstance(ss, int) else ss
        orig, mask = _as_model_domain(image), _as_binary_mask(mask_image)
        if tuple(orig.shape[1:]) != (c.in_channels, h, w):
            raise ValueError(f"RePaintPipeline: image has shape {tuple(orig.shape)}, the network takes "
                             f"[N, {c.in_channels}, {h}, {w}]")
        n = int(orig.shape[0])
        if batch_size is not None:
            if int(batch_size) < 1 or (n != 1 and n != int(batch_size)):
                raise ValueError(f"RePaintPipeline: batch_size={batch_size} with {n} images (one image, or one per sample)")
            n = int(batch_size)
        if (int(mask.shape[0]) not in (1, n) or int(mask.shape[1]) not in (1, c.in_channels)
                or tuple(mask.shape[2:]) != (h, w)):
            raise ValueError(f"RePaintPipeline: mask_image has shape {tuple(mask.shape)}, expected "
                             f"[{n} or 1, {c.in_channels} or 1, {h}, {w}]")
        return orig, mask, (n, c.in_channels, h, w)

    @torch.no_grad()
    def __call__(self, image, mask_image, num_inference_steps: int = 250, eta: float = 0.0, jump_length: int = 10,
                 jump_n_sample: int = 10, generator=None, output_type="pil", return_dict: bool = True, batch_size=None,
                 noise: str = "host", seed=None):
        """`batch_size=K` with one `image`: K different completions of one scene (the original and the mask are shared by the
        batch through the kernel's broadcast; diffusers has no such argument).  ``noise="device", seed=S``: no host draw at
        all -- x_T and every later draw are the Philox tensors (S, 0), (S, 1), ... (``RePaintScheduler.use_device_noise``:
        the same distribution as the default, not the same values; `generator` is not touched)."""
        if noise not in ("host", "device"):
            raise ValueError(f"RePaintPipeline: noise={noise!r} (supported: 'host', 'device')")
        if noise == "device" and seed is None:
            raise ValueError("RePaintPipeline: noise='device' needs seed=<int>")
        orig, mask, full = self._check_inputs(image, mask_image, batch_size)
        if self.device.type != "cuda":
            raise RuntimeError("RePaintPipeline runs on the MI355X HIP engine only: call .to('cuda') first")
        sch = self.scheduler
        with torch.cuda.device(self.device):
            orig, mask = orig.to(self.device), mask.to(self.device)
            sch.set_timesteps(num_inference_steps, jump_length, jump_n_sample)
            sch.eta = float(eta)
            ts = [int(t) for t in sch.timesteps]
            ratio = sch.config.num_train_timesteps // sch.num_inference_steps
            t_last = ts[0] + 1
            plan = []                                  # True: U-Net + step, False: undo (diffusers' loop, decided up front)
            for t in ts:
                plan.append(t < t_last)
                t_last = t
            stream = None
            try:
                if noise == "device":
                    sch.use_device_noise(seed)
                    x = sch.device_randn(full, self.device)
                    draw = None
                else:
                    sch.use_host_noise()
                    stream = _NoiseStream(full, generator, self.device,
                                          count=1 + sum(1 if fwd else ratio for fwd in plan))
                    x, draw = stream.draw(), stream.draw
                tdev = _device_timestep_rows(sch.timesteps, full[0], self.device)
                t_last = ts[0] + 1
                for i, t in enumerate(ts):
                    if plan[i]:
                        eps = self.unet(x, tdev[i]).sample
                        x = sch.step(eps, t, x, orig, mask, variance_noise=draw() if draw else None).prev_sample
                    else:
                        x = sch.undo_step(x, t_last, variance_noise=draw)
                    t_last = t
            finally:
                if stream is not None:
                    stream.close()
                sch.use_host_noise()
        return self._finish(x, output_type, return_dict)
