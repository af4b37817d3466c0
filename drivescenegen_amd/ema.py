"""``EMAModel``: exponential moving average of a model's weights, the diffusers 0.20.0 ``training_utils.EMAModel`` protocol
(constructor, ``get_decay``, ``step``, ``copy_to``, ``store`` / ``restore``, ``state_dict`` / ``load_state_dict``, ``to``,
``save_pretrained`` / ``from_pretrained``) -- what diffusers' own ``train_unconditional.py`` keeps next to the loop the
reference's training_pipeline.py:46-107 is a trimmed copy of.

Host logic only; the arithmetic is ONE ``dsg_ema_step`` launch per step (csrc/ema.hip) over a cached device job table:
  * the shadows live in one flat fp32 buffer, slices 64-element aligned in parameter order (``TrainState``'s rule), so that
    once ``AdamW`` has moved the live parameters into its slab -- same rule, same order -- the table is a single job;
  * the table is rebuilt whenever a parameter's ``data_ptr()``, ``requires_grad`` or the parameter count changed
    (``AdamW``'s first step moves every ``p.data``);
  * ``copy_to`` / ``restore`` write behind autograd's back and bump every written parameter's version counter, which is
    what ``UNet2DModel``'s plan and the training tape's weight packs are refreshed by.
Out of scope: 0.20.0's deprecated ``max_value`` / ``min_value`` / ``device`` keywords and the later ``foreach`` option
(``TypeError``), and a Module in place of the parameters.
"""
from __future__ import annotations

import copy
import json
import os

import numpy as np
import torch

from . import ops

_ALIGN = 64  # elements: 256-B aligned slices, as autograd.TrainState lays out the gradient (and AdamW the parameter) slab
_SCALARS = ("decay", "min_decay", "optimization_step", "update_after_step", "use_ema_warmup", "inv_gamma", "power")


def _checked(parameters, what):
    if isinstance(parameters, torch.nn.Module):
        raise TypeError(f"EMAModel{what}: pass model.parameters(), not the Module (the form diffusers 0.20.0 deprecates)")
    parameters = list(parameters)
    for p in parameters:
        if not isinstance(p, torch.Tensor):
            raise TypeError(f"EMAModel{what}: expected tensors, got {type(p).__name__}")
        if p.dtype != torch.float32:
            raise RuntimeError(f"drivescenegen_amd.EMAModel{what}: parameters must be fp32 (got {p.dtype})")
        if not p.is_cuda:
            raise RuntimeError(f"drivescenegen_amd.EMAModel{what}: the HIP engine needs GPU tensors (got a CPU tensor); "
                               "there is no CPU fallback")
    return parameters


class EMAModel:
    """Exponential Moving Average of model weights (diffusers 0.20.0 ``EMAModel``), averaged by one fused kernel."""

    def __init__(self, parameters, decay: float = 0.9999, min_decay: float = 0.0, update_after_step: int = 0,
                 use_ema_warmup: bool = False, inv_gamma: float = 1.0, power: float = 2 / 3, model_cls=None,
                 model_config=None):
        parameters = _checked(parameters, "")
        if not parameters:
            raise ValueError("EMAModel: no parameters")
        self._shapes = [tuple(p.shape) for p in parameters]
        self._numels = [p.numel() for p in parameters]
        self._offsets, off = [], 0
        for n in self._numels:
            self._offsets.append(off)
            off += (n + _ALIGN - 1) // _ALIGN * _ALIGN
        self._flat = torch.zeros(off, dtype=torch.float32, device=parameters[0].device)   # (the padding stays zero)
        self._make_views()
        with torch.no_grad():
            for s, p in zip(self.shadow_params, parameters):
                s.copy_(p.detach())
        self.temp_stored_params = None
        self._stored_flat = None
        self.decay, self.min_decay, self.update_after_step = decay, min_decay, update_after_step
        self.use_ema_warmup, self.inv_gamma, self.power = use_ema_warmup, inv_gamma, power
        self.optimization_step = 0
        self.cur_decay_value = None  # set in `step()`
        self.model_cls, self.model_config = model_cls, model_config
        self._table = self._table_key = self._param_flat = None

    def _make_views(self):
        self.shadow_params = [self._flat[o:o + n].view(sh) for o, n, sh in zip(self._offsets, self._numels, self._shapes)]

    # ---- decay schedule: Python doubles, diffusers' expressions ----------------------------------
    def get_decay(self, optimization_step: int) -> float:
        step = max(0, optimization_step - self.update_after_step - 1)
        if step <= 0:
            return 0.0
        if self.use_ema_warmup:
            cur_decay_value = 1 - (1 + step / self.inv_gamma) ** -self.power
        else:
            cur_decay_value = (1 + step) / (10 + step)
        cur_decay_value = min(cur_decay_value, self.decay)
        cur_decay_value = max(cur_decay_value, self.min_decay)
        return cur_decay_value

    # ---- job table --------------------------------------------------------------------------------
    def _pad_index(self):
        idx = [torch.arange(o + n, o2) for o, n, o2 in zip(self._offsets, self._numels, self._offsets[1:])]
        return torch.cat(idx) if idx else torch.zeros(0, dtype=torch.long)

    def _slab_view(self, parameters):
        """If the parameters are slices of ONE storage at the shadow buffer's own relative offsets and the elements between
        them are zero (AdamW's slab, padding included): a flat view of that storage from parameter 0 to the end of the
        last parameter.  The job of a slice may then run over the padding behind it -- owned by the slab on one side, by the
        shadow buffer on the other, zero on both and zero afterwards -- and the table merges into one job."""
        p0 = parameters[0]
        st = p0.untyped_storage()
        for p, o in zip(parameters, self._offsets):
            if p.untyped_storage().data_ptr() != st.data_ptr() or not p.is_contiguous() or p.data_ptr() - p0.data_ptr() != 4 * o:
                return None
        span = self._offsets[-1] + self._numels[-1]
        flat = torch.empty(0, dtype=torch.float32, device=p0.device).set_(st, (p0.data_ptr() - st.data_ptr()) // 4, (span,))
        pad = self._pad_index().to(p0.device)
        if pad.numel() and bool(flat[pad].ne(0).any()):
            return None
        return flat

    def _ensure_table(self, parameters):
        key = tuple((p.data_ptr(), p.requires_grad) for p in parameters)
        if self._table is not None and key == self._table_key:
            return self._table
        if len(parameters) != len(self.shadow_params):
            raise ValueError(f"EMAModel: {len(parameters)} parameters for {len(self.shadow_params)} shadow parameters")
        for p, s in zip(parameters, self.shadow_params):
            if tuple(p.shape) != tuple(s.shape) or p.device != s.device:
                raise ValueError(f"EMAModel: parameter {tuple(p.shape)} on {p.device} does not match its shadow "
                                 f"{tuple(s.shape)} on {s.device}")
        self._param_flat = self._slab_view(parameters)
        if self._param_flat is not None:   # every job but the last runs to the next slice
            ends = self._offsets[1:] + [self._offsets[-1] + self._numels[-1]]
            extents = [e - o for o, e in zip(self._offsets, ends)]
        else:
            extents = self._numels
            if not all(p.is_contiguous() for p in parameters):
                raise RuntimeError("drivescenegen_amd.EMAModel: parameters must be contiguous")
        jobs = [(p.data_ptr(), self._flat.data_ptr() + 4 * o, n, not rg)
                for p, o, n, (_, rg) in zip(parameters, self._offsets, extents, key) if n]
        self._table = ops.EmaTable(jobs, self._flat.device)
        self._table_key = key
        return self._table

    def _single_job(self, parameters):
        """The flat view of the live parameters when ONE copy moves all of them, else None."""
        table = self._ensure_table(parameters)
        return self._param_flat if self._param_flat is not None and table.n == 1 else None

    # ---- the protocol -----------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, parameters):
        parameters = _checked(parameters, ".step")
        self.optimization_step += 1
        decay = self.get_decay(self.optimization_step)
        self.cur_decay_value = decay
        self._ensure_table(parameters).run(np.float32(1 - decay))

    @staticmethod
    def _bump_versions(parameters):
        for p in parameters:
            torch.autograd.graph.increment_version(p)

    @torch.no_grad()
    def copy_to(self, parameters) -> None:
        """Copy the averaged weights into `parameters` (a device copy; one copy when the job table is a single job)."""
        parameters = _checked(parameters, ".copy_to")
        flat = self._single_job(parameters)
        if flat is not None:
            flat.copy_(self._flat[:flat.numel()])
        else:
            for s, p in zip(self.shadow_params, parameters):
                p.data.copy_(s)
        self._bump_versions(parameters)

    @torch.no_grad()
    def store(self, parameters) -> None:
        """Save the current parameters for `restore`.  The clones stay on the DEVICE (diffusers 0.20.0 moves them to the
        CPU): a 56.6-M-parameter network is 226 MB on a 288-GB part, and the round trip would cost two host copies per
        evaluation."""
        parameters = _checked(parameters, ".store")
        flat = self._single_job(parameters)
        if flat is not None:
            self._stored_flat = flat.clone()
            self.temp_stored_params = [self._stored_flat[o:o + n].view(sh)
                                       for o, n, sh in zip(self._offsets, self._numels, self._shapes)]
        else:
            self._stored_flat = None
            self.temp_stored_params = [p.detach().clone() for p in parameters]

    @torch.no_grad()
    def restore(self, parameters) -> None:
        """Put the parameters saved by `store` back (and forget them): training goes on from the raw weights."""
        if self.temp_stored_params is None:
            raise RuntimeError("This ExponentialMovingAverage has no `store()`ed weights to `restore()`")
        parameters = _checked(parameters, ".restore")
        flat = self._single_job(parameters) if self._stored_flat is not None else None
        if flat is not None and flat.numel() == self._stored_flat.numel():
            flat.copy_(self._stored_flat)
        else:
            for c, p in zip(self.temp_stored_params, parameters):
                p.data.copy_(c)
        self._bump_versions(parameters)
        self.temp_stored_params = self._stored_flat = None

    def to(self, device=None, dtype=None) -> None:
        """Move the shadow buffer (and a stored copy) to `device`; the dtype stays fp32."""
        if dtype not in (None, torch.float32):
            raise RuntimeError(f"drivescenegen_amd.EMAModel.to: the shadows stay fp32 (got dtype={dtype})")
        if device is None:
            return
        if torch.device(device).type != "cuda":
            raise RuntimeError("drivescenegen_amd.EMAModel.to: the HIP engine needs GPU tensors; there is no CPU fallback")
        self._flat = self._flat.to(device)
        self._make_views()
        if self.temp_stored_params is not None:
            self.temp_stored_params = [c.to(device) for c in self.temp_stored_params]
            self._stored_flat = None
        self._table = self._table_key = self._param_flat = None

    def state_dict(self) -> dict:
        return {"decay": self.decay, "min_decay": self.min_decay, "optimization_step": self.optimization_step,
                "update_after_step": self.update_after_step, "use_ema_warmup": self.use_ema_warmup,
                "inv_gamma": self.inv_gamma, "power": self.power, "shadow_params": self.shadow_params}

    def load_state_dict(self, state_dict: dict) -> None:
        state_dict = copy.deepcopy(state_dict)
        self.decay = state_dict.get("decay", self.decay)
        if self.decay < 0.0 or self.decay > 1.0:
            raise ValueError("Decay must be between 0 and 1")
        self.min_decay = state_dict.get("min_decay", self.min_decay)
        if not isinstance(self.min_decay, float):
            raise ValueError("Invalid min_decay")
        self.optimization_step = state_dict.get("optimization_step", self.optimization_step)
        if not isinstance(self.optimization_step, int):
            raise ValueError("Invalid optimization_step")
        self.update_after_step = state_dict.get("update_after_step", self.update_after_step)
        if not isinstance(self.update_after_step, int):
            raise ValueError("Invalid update_after_step")
        self.use_ema_warmup = state_dict.get("use_ema_warmup", self.use_ema_warmup)
        if not isinstance(self.use_ema_warmup, bool):
            raise ValueError("Invalid use_ema_warmup")
        self.inv_gamma = state_dict.get("inv_gamma", self.inv_gamma)
        if not isinstance(self.inv_gamma, (float, int)):
            raise ValueError("Invalid inv_gamma")
        self.power = state_dict.get("power", self.power)
        if not isinstance(self.power, (float, int)):
            raise ValueError("Invalid power")
        shadow_params = state_dict.get("shadow_params", None)
        if shadow_params is not None:
            if not isinstance(shadow_params, list):
                raise ValueError("shadow_params must be a list")
            if not all(isinstance(p, torch.Tensor) for p in shadow_params):
                raise ValueError("shadow_params must all be Tensors")
            if [tuple(p.shape) for p in shadow_params] != self._shapes:
                raise ValueError("shadow_params do not match the shapes this EMAModel was built for")
            with torch.no_grad():   # into the flat buffer: the views, and a cached job table, stay valid
                for s, p in zip(self.shadow_params, shadow_params):
                    s.copy_(p.to(torch.float32))

    # ---- checkpoint folder ------------------------------------------------------------------------
    def save_pretrained(self, path):
        """A model of `model_cls` built from `model_config` with the averaged weights, saved with its own
        ``save_pretrained``; the seven scalars go into that folder's config.json (where diffusers' ``register_to_config``
        puts them), so the folder also loads as a plain model."""
        if self.model_cls is None:
            raise ValueError("`save_pretrained` can only be used if `model_cls` was defined at __init__.")
        if self.model_config is None:
            raise ValueError("`save_pretrained` can only be used if `model_config` was defined at __init__.")
        cfg = self.model_config.to_dict() if hasattr(self.model_config, "to_dict") else dict(self.model_config)
        cfg = {k: v for k, v in cfg.items() if not k.startswith("_")}
        model = self.model_cls.from_config(cfg) if hasattr(self.model_cls, "from_config") else self.model_cls(**cfg)
        model.to(self._flat.device)
        self.copy_to(model.parameters())
        model.save_pretrained(path)
        config_file = os.path.join(path, getattr(self.model_cls, "config_name", "config.json"))
        with open(config_file) as f:
            saved = json.load(f)
        state = self.state_dict()
        saved.update({k: state[k] for k in _SCALARS})
        with open(config_file, "w") as f:
            json.dump(saved, f, indent=2, sort_keys=True)
            f.write("\n")

    @classmethod
    def from_pretrained(cls, path, model_cls, device=None) -> "EMAModel":
        """The EMA of a folder written by `save_pretrained`: shadows from the model's weights (moved to `device`, default
        the current GPU), the seven scalars from its config.json."""
        with open(os.path.join(path, getattr(model_cls, "config_name", "config.json"))) as f:
            saved = json.load(f)
        model = model_cls.from_pretrained(path)
        model.to(torch.device("cuda", torch.cuda.current_device()) if device is None else device)
        ema_model = cls(model.parameters(), model_cls=model_cls, model_config=model.config)
        ema_model.load_state_dict({k: saved[k] for k in _SCALARS if k in saved})
        return ema_model
