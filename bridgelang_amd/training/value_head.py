"""The critic's parameters: a linear value head V(s) = w·hn + b on the decoder's final-norm output (an `nn.Linear(D, 1)`),
trained with the policy by `TrainStep(loss="policy", value=ValueLossConfig(...))` (training/value_loss.py is the loss).

The head's two tensors are live bf16 device tensors, as LoRA's adapters are: the step's ParamStore carries them as extra
units (fp32 masters, AdamW moments, clipping, write-back, sharding), and the value kernels read them in place."""
from __future__ import annotations

from pathlib import Path
from typing import Dict, List, Optional, Tuple

import torch

WEIGHT, BIAS = "value_head.weight", "value_head.bias"
FILE_NAME = "value_head.safetensors"


class ValueHead:
    def __init__(self, dim: int, device, init_std: float = 0.0, seed: int = 0):
        """Zero-initialised by default: a fresh head predicts 0 everywhere and adds nothing to the trunk's first gradient
        (dhn += dv·w with w = 0). `init_std` > 0 draws the weight from N(0, init_std²) with the host generator `seed`."""
        if dim < 8 or dim % 8:
            raise ValueError(f"ValueHead: dim must be a positive multiple of 8, got {dim}")
        self.dim, self.device = int(dim), torch.device(device)
        w = torch.zeros(dim, dtype=torch.float32)
        if init_std:
            w = torch.randn(dim, generator=torch.Generator().manual_seed(seed)) * float(init_std)
        self.weight = w.to(self.device, torch.bfloat16).contiguous()
        self.bias = torch.zeros(1, dtype=torch.bfloat16, device=self.device)

    def plain_units(self) -> List[Tuple[str, torch.Tensor, bool, str]]:
        """(name, live bf16 tensor, weight-decayed, bucket) for the ParamStore, as `LoraAdapters.plain_units()`: the weight is
        a Linear weight and decays, the bias does not (fsdp.py:208), so each gets a bucket of its own (one decay class per
        bucket). Neither bucket is parameter-sharded: every rank keeps the head."""
        return [(WEIGHT, self.weight.view(-1), True, WEIGHT), (BIAS, self.bias.view(-1), False, BIAS)]

    def state_dict(self, masters: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """fp32 CPU tensors under the names of an `nn.Linear(D, 1)` called `value_head`: weight [1, D], bias [1]. `masters`
        (`store.master_state_dict()`) replaces the live bf16 values with the optimizer's fp32 masters."""
        src = masters if masters else {WEIGHT: self.weight, BIAS: self.bias}
        return {WEIGHT: src[WEIGHT].detach().float().cpu().reshape(1, self.dim).clone(),
                BIAS: src[BIAS].detach().float().cpu().reshape(1).clone()}

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> "ValueHead":
        """Into the live tensors, in place (a step planned over this head keeps reading them). An optimizer's masters are
        not touched: build the step after loading."""
        w, b = sd[WEIGHT], sd[BIAS]
        if w.numel() != self.dim or tuple(w.shape) not in ((1, self.dim), (self.dim,)) or b.numel() != 1:
            raise ValueError(f"ValueHead: {WEIGHT} {tuple(w.shape)} / {BIAS} {tuple(b.shape)}, expected (1, {self.dim}) / (1,)")
        self.weight.copy_(w.reshape(-1).to(self.device, torch.bfloat16))
        self.bias.copy_(b.reshape(-1).to(self.device, torch.bfloat16))
        return self

    def save(self, directory, masters: Optional[Dict[str, torch.Tensor]] = None) -> Path:
        """One file, `value_head.safetensors`, in `directory` (next to an adapter directory's files, or a run's own)."""
        from safetensors.torch import save_file
        d = Path(directory)
        d.mkdir(parents=True, exist_ok=True)
        save_file({k: v.contiguous() for k, v in self.state_dict(masters).items()}, str(d / FILE_NAME))
        return d / FILE_NAME

    @classmethod
    def load(cls, directory, device) -> "ValueHead":
        from safetensors.torch import load_file
        path = Path(directory) / FILE_NAME
        if not path.exists():
            raise FileNotFoundError(f"{path}: no value head saved here")
        sd = load_file(str(path))
        return cls(sd[WEIGHT].numel(), device).load_state_dict(sd)
