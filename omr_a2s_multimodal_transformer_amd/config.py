"""Model configuration (HF-style to_dict/from_dict/save/load surface).

The reference hard-codes its hyper-parameters (decoder.py:61-68: embedding_dim=256,
ff_dim=256, nhead=4, num_transformer_layers=8, dropout_p=0.1; encoder.py:251 dropout=0.5;
model.py:95-96 num_channels=256).  Defaults here equal those values; BASELINE.json's
"2-layer d_model=128" and "6-layer d_model=256" configs are reached by overriding them.
"""
from __future__ import annotations

import json
import math
from dataclasses import asdict, dataclass, fields
from typing import Any, Dict, Optional, Tuple


@dataclass
class ModelConfig:
    d_model: int = 256          # decoder.py:61 embedding_dim / encoder.py:267 last DSCBlock width
    nhead: int = 4              # decoder.py:66
    ff_dim: int = 256           # decoder.py:64
    num_layers: int = 8         # decoder.py:67
    dropout: float = 0.1        # decoder.py:65, model.py:29 (PE dropouts)
    encoder_dropout: float = 0.5  # encoder.py:251
    compute_dtype: str = "fp32"   # "fp32" (parity mode) or "bf16" (fp32 master weights + Adam)
    fp8_decode: bool = False      # BASELINE config 5 (extension): greedy / beam decode with fp8 (e4m3) MFMA weights in the decoder
    label_smoothing: float = 0.0  # extension: CrossEntropyLoss(label_smoothing=...) in training, torch's definition and range [0, 1]
    ctc_weight: float = 0.0       # extension: w in [0, 1] of loss = (1 - w) CE + w CTC; > 0 gives Transformer a CTC head on the encoder memory
    ctc_pool: int = 1             # extension: feature-grid rows averaged into one CTC frame (>= 1): divides the head's cost

    def __post_init__(self) -> None:
        w, p = self.ctc_weight, self.ctc_pool
        if isinstance(w, bool) or not isinstance(w, (int, float)) or not 0.0 <= w <= 1.0:       # NaN fails
            raise ValueError(f"ModelConfig: ctc_weight must lie in [0, 1] (got {w!r})")
        if isinstance(p, bool) or not isinstance(p, int) or p < 1:
            raise ValueError(f"ModelConfig: ctc_pool must be an integer >= 1 (got {p!r})")
        self.ctc_weight = float(w)

    def to_dict(self) -> Dict[str, Any]:
        return asdict(self)

    @classmethod
    def from_dict(cls, d: Dict[str, Any]) -> "ModelConfig":
        names = {f.name for f in fields(cls)}
        return cls(**{k: v for k, v in d.items() if k in names})

    def save_pretrained(self, path: str) -> None:
        with open(path, "w") as f:
            json.dump(self.to_dict(), f, indent=2)

    @classmethod
    def from_pretrained(cls, path: str) -> "ModelConfig":
        with open(path) as f:
            return cls.from_dict(json.load(f))


SCHEDULES = ("constant", "linear", "cosine")


@dataclass
class OptimConfig:
    """The optimizer recipe of params.FusedAdam (an extension: the reference trains with torch.optim.Adam(lr=1e-4) alone,
    model.py:134-139; the defaults here are that optimizer).  Decoupled weight decay is torch.optim.AdamW's, the average is
    torch.optim.swa_utils' get_ema_multi_avg_fn, the schedule is lr_at below."""
    lr: float = 1e-4
    betas: Tuple[float, float] = (0.9, 0.999)
    eps: float = 1e-8
    weight_decay: float = 0.0            # decoupled (AdamW): p *= 1 - lr * weight_decay in front of the Adam update
    no_decay: Tuple[str, ...] = ("bias", "norm")   # parameters whose name holds one of these never decay; nor does any with dim() < 2
    warmup_steps: int = 0                # linear warm-up: lr * (k + 1) / warmup_steps for call k < warmup_steps
    schedule: str = "constant"           # after the warm-up: "constant", or "linear" / "cosine" from lr to lr * min_lr_ratio at total_steps
    total_steps: Optional[int] = None    # needed by "linear" and "cosine"
    min_lr_ratio: float = 0.0
    ema_decay: Optional[float] = None    # None: no average; else ema = d * ema + (1 - d) * p after every applied step

    def __post_init__(self) -> None:
        self.betas = tuple(float(b) for b in self.betas)
        self.no_decay = (self.no_decay,) if isinstance(self.no_decay, str) else tuple(self.no_decay)
        if not (math.isfinite(self.lr) and self.lr >= 0):
            raise ValueError(f"OptimConfig: lr must be finite and >= 0 (got {self.lr})")
        if len(self.betas) != 2 or not all(0 <= b < 1 for b in self.betas):
            raise ValueError(f"OptimConfig: betas must be two values in [0, 1) (got {self.betas})")
        if not (math.isfinite(self.eps) and self.eps >= 0):
            raise ValueError(f"OptimConfig: eps must be finite and >= 0 (got {self.eps})")
        if not (math.isfinite(self.weight_decay) and self.weight_decay >= 0):
            raise ValueError(f"OptimConfig: weight_decay must be finite and >= 0 (got {self.weight_decay})")
        if not all(isinstance(s, str) and s for s in self.no_decay):
            raise ValueError(f"OptimConfig: no_decay must hold non-empty name substrings (got {self.no_decay})")
        if not (isinstance(self.warmup_steps, int) and self.warmup_steps >= 0):
            raise ValueError(f"OptimConfig: warmup_steps must be an integer >= 0 (got {self.warmup_steps})")
        if self.schedule not in SCHEDULES:
            raise ValueError(f"OptimConfig: schedule must be one of {SCHEDULES} (got {self.schedule!r})")
        if self.total_steps is not None and not (isinstance(self.total_steps, int) and self.total_steps >= 1):
            raise ValueError(f"OptimConfig: total_steps must be an integer >= 1 or None (got {self.total_steps})")
        if self.schedule != "constant":
            if self.total_steps is None:
                raise ValueError(f"OptimConfig: schedule={self.schedule!r} needs total_steps")
            if self.total_steps <= self.warmup_steps:
                raise ValueError(f"OptimConfig: total_steps ({self.total_steps}) must exceed warmup_steps ({self.warmup_steps})")
        if not (math.isfinite(self.min_lr_ratio) and 0 <= self.min_lr_ratio <= 1):
            raise ValueError(f"OptimConfig: min_lr_ratio must lie in [0, 1] (got {self.min_lr_ratio})")
        if self.ema_decay is not None and not 0 <= self.ema_decay <= 1:
            raise ValueError(f"OptimConfig: ema_decay must lie in [0, 1] or be None (got {self.ema_decay})")

    @property
    def plain(self) -> bool:
        """Asks for nothing beyond Adam at a constant rate: FusedAdam then launches what it launches without a config."""
        return self.weight_decay == 0 and self.ema_decay is None and self.schedule == "constant" and self.warmup_steps == 0

    def to_dict(self) -> Dict[str, Any]:
        d = asdict(self)
        d["betas"], d["no_decay"] = list(self.betas), list(self.no_decay)      # plain data: JSON and weights_only checkpoints
        return d

    @classmethod
    def from_dict(cls, d: Dict[str, Any]) -> "OptimConfig":
        names = {f.name for f in fields(cls)}
        return cls(**{k: v for k, v in d.items() if k in names})


@dataclass
class DistillConfig:
    """Knowledge distillation (distill.Distillation; an extension: the reference trains from hard labels alone).  The training loss is
    (1 - weight) nll + weight temperature^2 KL(q || softmax(student / temperature)) with the teachers' mix
    q = alpha softmax(a / temperature) + (1 - alpha) softmax(b / temperature); a single teacher is taken with alpha = 1."""
    weight: float = 0.5                  # share of the distillation term; 0 is the plain loss
    temperature: float = 2.0
    alpha: float = 0.5                   # weight of the first teacher (the image model of a cross-modal pair), as in the weighted late fusion

    def __post_init__(self) -> None:
        for name in ("weight", "temperature", "alpha"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)):
                raise ValueError(f"DistillConfig: {name} must be a number (got {v!r})")
            setattr(self, name, float(v))
        if not 0.0 <= self.weight <= 1.0:
            raise ValueError(f"DistillConfig: weight must lie in [0, 1] (got {self.weight})")
        if not (math.isfinite(self.temperature) and self.temperature > 0):
            raise ValueError(f"DistillConfig: temperature must be finite and > 0 (got {self.temperature})")
        if not 0.0 <= self.alpha <= 1.0:
            raise ValueError(f"DistillConfig: alpha must lie in [0, 1] (got {self.alpha})")

    def to_dict(self) -> Dict[str, Any]:
        return asdict(self)

    @classmethod
    def from_dict(cls, d: Dict[str, Any]) -> "DistillConfig":
        names = {f.name for f in fields(cls)}
        return cls(**{k: v for k, v in d.items() if k in names})


def lr_at(cfg: OptimConfig, k: int) -> float:
    """Learning rate of the k-th step() CALL (k = 0, 1, ...), in fp64 on the host.  Calls, not applied steps: a step the guard
    skips on the device still advances the schedule, so the host never waits for the decision.
      k < warmup_steps:   lr * (k + 1) / warmup_steps                       (linear; reaches lr at k = warmup_steps - 1)
      then "constant":    lr
           "linear":      lr * (r + (1 - r) * (1 - t))                      r = min_lr_ratio,
           "cosine":      lr * (r + (1 - r) * (1 + cos(pi t)) / 2)          t = (k - warmup_steps) / (total_steps - warmup_steps)
      k >= total_steps:   lr * r, held                                      (t = 1)"""
    if k < 0:
        raise ValueError(f"lr_at: k must be >= 0 (got {k})")
    if k < cfg.warmup_steps:
        return cfg.lr * (k + 1) / cfg.warmup_steps
    if cfg.schedule == "constant":
        return cfg.lr
    t = min(1.0, (k - cfg.warmup_steps) / (cfg.total_steps - cfg.warmup_steps))
    r = cfg.min_lr_ratio
    shape = 1.0 - t if cfg.schedule == "linear" else 0.5 * (1.0 + math.cos(math.pi * t))
    return cfg.lr * (r + (1.0 - r) * shape)


# BASELINE.json configs (SURVEY.md section 8 "Configs")
C1_TINY = ModelConfig(d_model=128, nhead=4, ff_dim=128, num_layers=2)
C2_IMAGE = ModelConfig(d_model=256, nhead=4, ff_dim=256, num_layers=6, compute_dtype="bf16")
REFERENCE_DEFAULT = ModelConfig()
