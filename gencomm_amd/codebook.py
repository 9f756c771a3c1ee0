"""The CodeFilling codebook codec: ``UMGMQuantizer`` (opencood/models/sub_modules/codebook.py:280) on one fused HIP kernel.

A 1..3-level residual multi-codebook quantizer applied to every BEV pixel (row of ``channel`` values) of every agent. The baseline
``heter_model_baseline_w_codebook`` transmits its codes -- ``len(k) * m * log2 k`` bits per pixel -- where GenComm transmits a
2-channel message. This module is the component, for inference; the baseline's shell (``Communication``, the
``point_pillar_codebook_loss`` criterion) is not here.

Per level i the encoder computes ``z = E_i(x)``, ``h = Q_i(z)``, per group the logits ``-(|h_g - c|^2) / sqrt(k) * max(temperature_g,
1e-6)``, the sampled index ``argmax(logit + gumbel)`` and the returned code ``argmax(logit)``, and hands ``LH_i(z) - q_i`` to the next
level; the decoder runs ``f <- R_i(DH_i(q_i) + S_i(f))`` from the last level to the first. All of it is ONE launch of
``gencomm_umgm_fwd`` (csrc/codebook_kernels.h) plus a one-workgroup sum for ``code_loss``.

The ``state_dict`` has the reference's keys and shapes: a level's codebook is ONE parameter that appears as
``_encoders.i._quantizer._codebook``, ``_encoders.i._dequantizer._codebook`` and ``_decoders.i._dequantizer._codebook``; a reference
checkpoint loads with ``strict=True``.

Noise (the reference draws ``torch.rand_like`` per level inside ``gumbelSoftmax``): ``uniforms`` supplies the draws (a list of
``[n, m, k_i]`` float32 tensors, to which the kernel applies the reference's clamp and ``-log(-log u)``); otherwise they are drawn in
the kernel from a Philox stream keyed by ``seed`` (default: a seed from torch's default generator, so ``torch.manual_seed`` makes a
run reproducible; ``philox_uniforms(seed, n)`` exports the field); ``noise=False`` adds none: the sampled index is the code -- the
deterministic codec, and what ``decode(encode(x))`` restores.

Supported envelope: channel 64 | 128 | 256; m 1 | 2 | 4; 1..3 levels; each k a power of two in 16..256; every component an
``nn.Linear(channel, channel)``; ``permutationRate`` 0. By default inference only: a grad-enabled call that would need a gradient raises.

Training is opt-in: ``UMGMQuantizer(..., trainable=True)`` sends a grad-enabled ``forward`` / ``forward_map`` that needs a gradient through
``codebook_bwd.UMGMFunction`` -- the same forward launch, and the straight-through backward ``gencomm_umgm_bwd``. ``restored`` and
``code_loss`` are differentiable with respect to ``x``, the Linear heads, the tied codebooks and the temperatures; ``codes`` and ``logits``
are marked non-differentiable (the baseline's shell discards both). ``encode`` / ``decode`` / ``pack`` stay inference-only.
"""
from __future__ import annotations

import ctypes
import math
from typing import Callable, Dict, List, Optional, Sequence, Union

import torch
import torch.nn as nn

from . import _lib
from .runtime import f32c, ptr, require_gpu, stream_ptr, workspaces

COMPONENTS = ("latentStageEncoder", "quantizationHead", "latentHead", "dequantizationHead", "sideHead", "restoreHead")
CHANNELS, GROUPS, MAX_LEVELS = (64, 128, 256), (1, 2, 4), 3
_SLOTS = ("_latentStageEncoder", "_quantizationHead", "_latentHead", "_dequantizationHead", "_sideHead", "_restoreHead")   # blob order


# ----------------------------------------------------------------------------------------- parameter containers (the reference's tree)
class _Bound(nn.Module):      # codebook_utils.py:34 LowerBound: its `bound` buffer is part of the state_dict
    def __init__(self, bound):
        super().__init__()
        self.register_buffer("bound", torch.Tensor([float(bound)]))


class _Quantization(nn.Module):
    def __init__(self, codebook):
        super().__init__()
        self._codebook = codebook
        self._temperature = nn.Parameter(torch.ones((codebook.shape[0], 1)))
        self._bound = _Bound(1e-6)


class _DeQuantization(nn.Module):
    def __init__(self, codebook):
        super().__init__()
        self._codebook = codebook


class _Encoder(nn.Module):
    def __init__(self, quantizer, dequantizer, latentStageEncoder, quantizationHead, latentHead):
        super().__init__()
        self._quantizer, self._dequantizer = quantizer, dequantizer
        self._latentStageEncoder, self._quantizationHead, self._latentHead = latentStageEncoder, quantizationHead, latentHead


class _Decoder(nn.Module):
    def __init__(self, dequantizer, dequantizationHead, sideHead, restoreHead):
        super().__init__()
        self._dequantizer = dequantizer
        self._dequantizationHead, self._sideHead, self._restoreHead = dequantizationHead, sideHead, restoreHead


def _linear(components, key, channel):
    if key not in components:
        raise KeyError(f"UMGMQuantizer: components has no '{key}'")
    mod = components[key]()
    if type(mod) is not nn.Linear or mod.in_features != channel or mod.out_features != channel or mod.bias is None:
        raise NotImplementedError(f"UMGMQuantizer: component '{key}' must be nn.Linear({channel}, {channel}) with a bias "
                                  f"(got {mod}); the fused kernel runs the six heads of a level as {channel} x {channel} matrix products")
    return mod


class UMGMQuantizer(nn.Module):
    def __init__(self, channel: int, m: int, k: Union[int, List[int]], permutationRate: float,
                 components: Dict[str, Callable[[], nn.Module]], trainable: bool = False):
        super().__init__()
        self.trainable = bool(trainable)
        k = [k] if isinstance(k, int) else [int(v) for v in k]
        if channel not in CHANNELS:
            raise ValueError(f"UMGMQuantizer: channel {channel} is not supported (one of {list(CHANNELS)})")
        if m not in GROUPS:
            raise ValueError(f"UMGMQuantizer: m {m} is not supported (one of {list(GROUPS)})")
        if not 1 <= len(k) <= MAX_LEVELS:
            raise ValueError(f"UMGMQuantizer: k has {len(k)} levels (1 to {MAX_LEVELS} are supported)")
        for ki in k:
            if ki < 16 or ki > 256 or ki & (ki - 1):
                raise ValueError(f"UMGMQuantizer: k entry {ki} is not supported (a power of two in 16 .. 256)")
        if permutationRate > 0:
            raise NotImplementedError(f"UMGMQuantizer: permutationRate {permutationRate} is not supported (the reference's shell passes 0; "
                                      "the random permutation of samples is a training-time regulariser)")
        self._m, self._k, self._channel = m, k, channel
        encoders, decoders = [], []
        for i, ki in enumerate(k):
            last = i == len(k) - 1
            heads = {key: (None if last and key in ("latentHead", "sideHead") else _linear(components, key, channel)) for key in COMPONENTS}
            codebook = nn.Parameter(nn.init.normal_(torch.empty(m, ki, channel // m), std=math.sqrt(2 / (5 * channel / m))))
            quantizer, dequantizer = _Quantization(codebook), _DeQuantization(codebook)
            encoders.append(_Encoder(quantizer, dequantizer, heads["latentStageEncoder"], heads["quantizationHead"], heads["latentHead"]))
            decoders.append(_Decoder(dequantizer, heads["dequantizationHead"], heads["sideHead"], heads["restoreHead"]))
        self._encoders = nn.ModuleList(encoders)
        self._decoders = nn.ModuleList(decoders)
        self._blob, self._blob_key = None, None

    # ------------------------------------------------------------------------------------- properties
    @property
    def _k_arr(self):
        return (ctypes.c_int * len(self._k))(*self._k)

    @property
    def Codebooks(self):
        return [enc._quantizer._codebook for enc in self._encoders]

    @property
    def payload_bits_per_row(self) -> int:
        return sum(self._m * int(math.log2(ki)) for ki in self._k)

    @property
    def payload_bytes_per_row(self) -> int:
        return (self.payload_bits_per_row + 7) // 8

    # ------------------------------------------------------------------------------------- the parameter blob
    def _blob_tensors(self):
        out = []
        for enc, dec in zip(self._encoders, self._decoders):
            for name in _SLOTS:
                mod = getattr(enc, name, None) if hasattr(enc, name) else getattr(dec, name, None)
                if mod is None:
                    out.append(None)
                else:
                    out += [mod.weight, mod.bias]
            out += [enc._quantizer._codebook, enc._quantizer._temperature]
        return out

    def _params(self, device) -> torch.Tensor:
        """One flat float32 copy of every parameter in the kernel's order, rebuilt only when a parameter changed."""
        C, tensors = self._channel, self._blob_tensors()
        key = (str(device),) + tuple(None if t is None else (t.data_ptr(), t._version) for t in tensors)
        if key != self._blob_key or self._blob is None:
            parts = []
            with torch.no_grad():
                for t in tensors:
                    if t is None:                                      # the unread latentHead / sideHead slot of the last level
                        parts.append(torch.zeros(C * C + C, dtype=torch.float32, device=device))
                    elif t.dim() == 2 and t.shape[1] == 1:             # temperature [m, 1], padded to 4
                        parts.append(torch.cat([t.detach().reshape(-1).float(), torch.ones(4 - t.numel(), dtype=torch.float32, device=device)]))
                    else:
                        parts.append(t.detach().reshape(-1).float())
                blob = torch.cat(parts)
            want = _lib.check_size(_lib.lib().gencomm_umgm_param_floats(C, self._m, self._k_arr, len(self._k)), "gencomm_umgm_param_floats")
            assert blob.numel() == want, (blob.numel(), want)
            self._blob, self._blob_key = blob, key
        return self._blob

    # ------------------------------------------------------------------------------------- checks
    def _needs_grad(self, x):
        return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))

    def _refuse_grad(self, x):
        if self._needs_grad(x):
            raise NotImplementedError("UMGMQuantizer: codebook training is not implemented (the straight-through backward of the fused codec); "
                                      "call under torch.no_grad(), or freeze the parameters and detach the input")

    def _check_rows(self, x, what):
        require_gpu(x, f"UMGMQuantizer.{what}")
        if x.dim() != 2 or x.shape[1] != self._channel or x.shape[0] < 1:
            raise ValueError(f"UMGMQuantizer.{what}: x must be [n, {self._channel}] with n >= 1, got {list(x.shape)}")
        return f32c(x)

    def _check_map(self, x, what):
        require_gpu(x, f"UMGMQuantizer.{what}")
        if x.dim() != 4 or x.shape[1] != self._channel or x.shape[0] < 1 or x.shape[2] * x.shape[3] < 1:
            raise ValueError(f"UMGMQuantizer.{what}: x must be [agents, {self._channel}, H, W], got {list(x.shape)}")
        return f32c(x)

    def _noise_args(self, rows, uniforms, seed, noise, device):
        """(mode, uniforms tensor or None, seed)"""
        if uniforms is not None:
            if noise is False:
                raise ValueError("UMGMQuantizer: uniforms were given together with noise=False")
            if len(uniforms) != len(self._k):
                raise ValueError(f"UMGMQuantizer: uniforms has {len(uniforms)} entries for {len(self._k)} levels")
            flat = []
            for u, ki in zip(uniforms, self._k):
                if tuple(u.shape) != (rows, self._m, ki):
                    raise ValueError(f"UMGMQuantizer: a level's uniforms must be [{rows}, {self._m}, {ki}], got {list(u.shape)}")
                require_gpu(u, "UMGMQuantizer uniforms")
                flat.append(f32c(u).reshape(-1))
            return 1, (flat[0] if len(flat) == 1 else torch.cat(flat)), 0
        if noise is False:
            return 0, None, 0
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        return 2, None, int(seed)

    def _run(self, x, rows, HW, keep, uniforms, seed, noise, with_logits, with_sampled=False, noise_args=None):
        dev, l, L, m = x.device, _lib.lib(), len(self._k), self._m
        mode, u, seed = noise_args if noise_args is not None else self._noise_args(rows, uniforms, seed, noise, dev)
        restored = torch.empty_like(x)
        codes = torch.empty((L, rows, m), dtype=torch.int64, device=dev)
        sampled = torch.empty_like(codes) if with_sampled else None
        logits = torch.empty(rows * m * sum(self._k), dtype=torch.float32, device=dev) if with_logits else None
        loss = torch.empty((), dtype=torch.float32, device=dev)
        need = _lib.check_size(l.gencomm_umgm_workspace_bytes(rows, self._channel), "gencomm_umgm_workspace_bytes")
        ws = workspaces.get(dev, need, "umgm")
        n_arg = x.shape[0]
        _lib.check(l.gencomm_umgm_fwd(ptr(self._params(dev)), ptr(x), ptr(keep), ptr(u), seed, mode, ptr(restored), ptr(codes), ptr(sampled), ptr(logits), ptr(loss),
                                      n_arg, HW, self._channel, m, self._k_arr, L, ptr(ws), ws.numel(), stream_ptr(dev)), "gencomm_umgm_fwd")
        out_logits = None
        if with_logits:
            out_logits, off = [], 0
            for ki in self._k:
                out_logits.append(logits[off:off + rows * m * ki].view(rows, m, ki))
                off += rows * m * ki
        out = (restored, [codes[i] for i in range(L)], out_logits, loss)
        return out + ([sampled[i] for i in range(L)],) if with_sampled else out

    # ------------------------------------------------------------------------------------- the reference's interface
    def forward(self, x, uniforms: Optional[Sequence[torch.Tensor]] = None, seed: Optional[int] = None, noise: bool = True,
                return_sampled: bool = False):
        """x [n, channel] -> (restored [n, channel], codes: L x [n, m] int64, logits: L x [n, m, k_i], code_loss), as the reference;
        ``return_sampled`` appends the sampled indices (L x [n, m]), which the reference keeps to itself. With ``trainable=True`` and a
        gradient wanted, ``restored`` and ``code_loss`` carry it; ``codes`` and ``logits`` are non-differentiable."""
        if self.trainable and self._needs_grad(x):
            from .codebook_bwd import run_trainable
            require_gpu(x, "UMGMQuantizer.forward")
            return run_trainable(self, self._check_rows(x, "forward"), 0, None, uniforms, seed, noise, True, return_sampled)
        self._refuse_grad(x)
        x = self._check_rows(x, "forward")
        return self._run(x, x.shape[0], 0, None, uniforms, seed, noise, True, return_sampled)

    def forward_map(self, x_nchw, keep=None, uniforms: Optional[Sequence[torch.Tensor]] = None, seed: Optional[int] = None, noise: bool = True,
                    return_logits: bool = False):
        """The same over an NCHW map [agents, channel, H, W], read and written in place of the reference's two
        ``permute(...).contiguous()`` passes; row r of the rows entry is (agent, y, x) = (r // HW, (r % HW) // W, r % W). ``keep``: per-agent
        flags (bool tensor or sequence); a flagged agent's restored map is its input, bit for bit, while ``code_loss`` is the reference's
        (taken before the overwrite). Returns (restored NCHW, codes: L x [agents H W, m], logits or None, code_loss)."""
        train = self.trainable and self._needs_grad(x_nchw)
        if not train:
            self._refuse_grad(x_nchw)
        x = self._check_map(x_nchw, "forward_map")
        A, _, H, W = x.shape
        if keep is not None:
            keep = torch.as_tensor(keep).to(device=x.device, dtype=torch.uint8).contiguous()
            if keep.numel() != A:
                raise ValueError(f"UMGMQuantizer.forward_map: keep must have one flag per agent ({A}), got {keep.numel()}")
        if train:   # a kept agent's g_restored goes straight to dx; its rows still receive the code_loss gradient through the codec
            from .codebook_bwd import run_trainable
            return run_trainable(self, x, H * W, keep, uniforms, seed, noise, return_logits, False)
        return self._run(x, A * H * W, H * W, keep, uniforms, seed, noise, return_logits)

    def encode(self, x) -> List[torch.Tensor]:
        """The reference's ``encode``: per level the nearest codeword of every group (argmin of the distance), residuals carried."""
        self._refuse_grad(x)
        x = self._check_rows(x, "encode")
        dev, L, n = x.device, len(self._k), x.shape[0]
        codes = torch.empty((L, n, self._m), dtype=torch.int64, device=dev)
        _lib.check(_lib.lib().gencomm_umgm_encode_fwd(ptr(self._params(dev)), ptr(x), ptr(codes), n, 0, self._channel, self._m, self._k_arr, L,
                                                      stream_ptr(dev)), "gencomm_umgm_encode_fwd")
        return [codes[i] for i in range(L)]

    def decode(self, codes: Sequence[torch.Tensor]) -> torch.Tensor:
        """codes: L x [n, m] integers -> restored [n, channel] (the reference's ``decode`` with its ``_ix = arange(m)``)."""
        self._check_codes(codes)
        require_gpu(codes[0], "UMGMQuantizer.decode")
        dev, L, n = codes[0].device, len(self._k), codes[0].shape[0]
        stacked = torch.stack([c.to(torch.int64) for c in codes]).contiguous()
        lo, hi = stacked.amin(dim=(1, 2)).tolist(), stacked.amax(dim=(1, 2)).tolist()
        for i, ki in enumerate(self._k):
            if lo[i] < 0 or hi[i] >= ki:
                raise ValueError(f"UMGMQuantizer.decode: codes[{i}] has values in {lo[i]} .. {hi[i]}, outside the codebook 0 .. {ki - 1}")
        restored = torch.empty((n, self._channel), dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().gencomm_umgm_decode_fwd(ptr(self._params(dev)), ptr(stacked), ptr(restored), n, 0, self._channel, self._m, self._k_arr, L,
                                                      stream_ptr(dev)), "gencomm_umgm_decode_fwd")
        return restored

    def philox_uniforms(self, seed: int, n: int, device=None) -> List[torch.Tensor]:
        """The uniforms a ``forward(x, seed=seed)`` over n rows draws in the kernel (``gencomm_umgm_noise_fwd``): L x [n, m, k_i]."""
        dev = torch.device(device) if device is not None else next(self.parameters()).device
        if dev.type != "cuda":
            raise _lib.GenCommHipError(f"UMGMQuantizer.philox_uniforms: device {dev} is not a ROCm device")
        flat = torch.empty(n * self._m * sum(self._k), dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().gencomm_umgm_noise_fwd(ptr(flat), int(seed), n, self._m, self._k_arr, len(self._k), stream_ptr(dev)), "gencomm_umgm_noise_fwd")
        out, off = [], 0
        for ki in self._k:
            out.append(flat[off:off + n * self._m * ki].view(n, self._m, ki))
            off += n * self._m * ki
        return out

    # ------------------------------------------------------------------------------------- the payload
    def _check_codes(self, codes):
        if len(codes) != len(self._k):
            raise ValueError(f"UMGMQuantizer: codes has {len(codes)} entries for {len(self._k)} levels")
        n = codes[0].shape[0]
        for c in codes:
            if c.dim() != 2 or tuple(c.shape) != (n, self._m) or c.is_floating_point() or n < 1:
                raise ValueError(f"UMGMQuantizer: every level's codes must be integers [n, {self._m}] with one n >= 1, got {list(c.shape)} {c.dtype}")

    def pack(self, codes: Sequence[torch.Tensor]) -> torch.Tensor:
        """codes -> uint8 [n, ceil(L m log2 k / 8)]: level-major, group-minor bit fields, least significant bit first. Plain torch
        integer operations on the codes' device (the payload is 3 bytes per row at the shipped shape; not a hot path)."""
        self._check_codes(codes)
        n, dev = codes[0].shape[0], codes[0].device
        out = torch.zeros((n, self.payload_bytes_per_row), dtype=torch.int64, device=dev)
        pos = 0
        for c, ki in zip(codes, self._k):
            for g in range(self._m):
                field = c[:, g].to(torch.int64)
                for b in range(int(math.log2(ki))):
                    out[:, pos // 8] |= ((field >> b) & 1) << (pos % 8)
                    pos += 1
        return out.to(torch.uint8)

    def unpack(self, payload: torch.Tensor) -> List[torch.Tensor]:
        """uint8 [n, payload_bytes_per_row] -> codes (L x [n, m] int64), the inverse of ``pack``."""
        if payload.dim() != 2 or payload.shape[1] != self.payload_bytes_per_row or payload.dtype != torch.uint8:
            raise ValueError(f"UMGMQuantizer.unpack: payload must be uint8 [n, {self.payload_bytes_per_row}], got {list(payload.shape)} {payload.dtype}")
        p = payload.to(torch.int64)
        codes, pos = [], 0
        for ki in self._k:
            bits = int(math.log2(ki))
            level = torch.zeros((p.shape[0], self._m), dtype=torch.int64, device=p.device)
            for g in range(self._m):
                for b in range(bits):
                    level[:, g] |= ((p[:, (pos + b) // 8] >> ((pos + b) % 8)) & 1) << b
                pos += bits
            codes.append(level)
        return codes
