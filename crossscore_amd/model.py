"""Drop-in `CrossScoreNet` whose forward runs on the hand-written gfx950 kernels of libcrossscore_hip.so.

Mirrors the reference model boundary (task/core.py:26-161):
  * `CrossScoreNet(cfg)` reads the same config keys (config/model/model.yaml),
  * `state_dict()` has exactly the reference's keys and shapes, so a Lightning checkpoint's
    `ckpt["state_dict"]` (keys prefixed "model.") loads with `strict=True`,
  * `forward(query_img, ref_cross_imgs, need_attn_weights, need_attn_weights_head_id, norm_img)` returns
    `{"score_map_ref_cross": (B,14h,14w) fp32, "attn_weights_map_ref_cross": None | (B,h,w,N,h,w) fp32}`.
PyTorch is used here only for device buffers, the current stream and (de)serialisation: every arithmetic
stage of the forward is a HIP kernel launched through the C ABI.  There is no eager fallback.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import Any, Dict, Optional

import numpy as np
import torch

from . import _lib, synth
from .synth import ArchSpec, BACKBONES


# ----- config helpers restating utils/check_config.py:1-28 and model/regression_layer.py:31-62 ---------------
def check_metric_prediction_config(metric_type, metric_min, metric_max) -> None:
    if metric_type not in ("ssim", "mse", "mae"):
        raise ValueError(f"Invalid metric type {metric_type}")
    valid_max = metric_max == 1
    valid_min = (metric_min in (-1, 0)) if metric_type == "ssim" else (metric_min == 0)
    if not (valid_min and valid_max):
        raise ValueError(f"Invalid metric range {metric_min} to {metric_max} for {metric_type}")


def regression_activation(metric_type, metric_min, metric_max, power_factor):
    """-> (act, p): act 0 = sigmoid, 1 = tanh; p = exponent applied after the activation."""
    check_metric_prediction_config(metric_type, metric_min, metric_max)
    if metric_min == -1:
        act = 1
    elif metric_min == 0:
        act = 0
    else:
        raise ValueError(f"metric_min={metric_min} not supported")
    if metric_min == 0:
        p = {"ssim": 1, "mae": 2, "mse": 4}[metric_type] if power_factor == "default" else power_factor
    else:
        p = 1
    return act, float(p)


def arch_from_cfg(cfg) -> ArchSpec:
    """Architecture constants from cfg.model (the reference gets hidden size / layers / heads from
    Dinov2Config.from_pretrained(cfg.model.backbone.from_pretrained), task/core.py:39; the hub is unreachable
    offline, so the two published backbones are tabulated; cfg.model.backbone may also carry explicit
    hidden_size / num_hidden_layers / num_attention_heads / image_size)."""
    m = cfg.model
    bb = m.backbone
    name = bb.from_pretrained
    if name in BACKBONES:
        a = BACKBONES[name]
    elif all(k in bb for k in ("hidden_size", "num_hidden_layers", "num_attention_heads")):
        a = ArchSpec(hidden=int(bb.hidden_size), enc_layers=int(bb.num_hidden_layers), enc_heads=int(bb.num_attention_heads),
                     pos_grid=int(bb.get("image_size", 518)) // int(m.patch_size), name=str(name), swiglu=bool(bb.get("use_swiglu_ffn", False)))
    else:
        raise ValueError(f"unknown backbone '{name}': known {sorted(BACKBONES)} (or give explicit sizes in cfg.model.backbone)")
    return dataclasses.replace(a, patch=int(m.patch_size), pe_h=int(m.pos_enc.multi_view.h), pe_w=int(m.pos_enc.multi_view.w),
                               do_self_attn=bool(m.decoder_do_self_attn))


@dataclasses.dataclass(frozen=True)
class FitScope:
    """One scope of on-device fitting.  The scopes are nested through `parent`: a scope's tensors are its own, then its parent's
    (the order of its backward's gradients); its keep switch implies its parent's; its backward's workspace begins with its parent's.  `own`:
    the key suffixes of its own tensors behind `prefix` ({last} = the last decoder layer).  The rest are C names (include/crossscore_hip.h),
    the arch fields cs_*_fit_supported takes, and what check_fit_supported raises for another architecture."""
    name: str
    parent: Optional["FitScope"]
    prefix: str
    own: tuple
    supported: str
    supported_args: tuple
    keep: Optional[str]
    backward: str
    set_weights: str
    error: type
    built_for: str

    def chain(self):
        """this scope, its parent, ... down to the head"""
        s = self
        while s is not None:
            yield s
            s = s.parent

    def keys(self, dec_layers: int) -> tuple:
        return tuple(k for s in self.chain() for k in (s.prefix.format(last=dec_layers - 1) + o for o in s.own))


_LAST_LAYER = "ref_cross.attn.layers.{last}."
FIT_HEAD = FitScope("head", None, "ref_cross.head.", ("0.weight", "0.bias", "2.weight", "2.bias"), "cs_head_fit_supported", ("hidden", "patch"),
                    None, "cs_head_backward", "cs_set_head_weights", ValueError,
                    "head fit is built for hidden a multiple of 64 and patch 14 (hidden {a.hidden}, patch {a.patch})")
FIT_TAIL = FitScope("tail", FIT_HEAD, _LAST_LAYER, ("linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm3.weight", "norm3.bias"),
                    "cs_tail_fit_supported", ("hidden", "patch"), "cs_fit_tail_keep", "cs_tail_backward", "cs_set_tail_weights", ValueError,
                    "tail fit is built for hidden a multiple of 64 up to 2048 and patch 14 (hidden {a.hidden}, patch {a.patch})")
FIT_CROSS = FitScope("cross", FIT_TAIL, _LAST_LAYER, ("multihead_attn.in_proj_weight", "multihead_attn.in_proj_bias", "multihead_attn.out_proj.weight",
                                                      "multihead_attn.out_proj.bias", "norm2.weight", "norm2.bias"),
                     "cs_cross_fit_supported", ("hidden", "dec_heads", "patch"), "cs_fit_cross_keep", "cs_cross_backward", "cs_set_cross_weights",
                     NotImplementedError, "cross-attention fit is built for the tail's shapes and decoder head dims 16, 48 and 96 "
                                          "(hidden {a.hidden}, {a.dec_heads} heads, patch {a.patch})")
FIT_LAYER = FitScope("layer", FIT_CROSS, _LAST_LAYER, ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight",
                                                      "self_attn.out_proj.bias", "norm1.weight", "norm1.bias"),
                     "cs_layer_fit_supported", ("hidden", "dec_heads", "patch", "do_self_attn"), "cs_fit_layer_keep", "cs_layer_backward",
                     "cs_set_layer_weights", NotImplementedError, "whole-layer fit is built for the cross-attention fit's shapes "
                                                                  "(hidden {a.hidden}, {a.dec_heads} heads, patch {a.patch})")
FIT_SCOPES = {s.name: s for s in (FIT_HEAD, FIT_TAIL, FIT_CROSS, FIT_LAYER)}  # the one table: every lookup by name goes through it


def check_fit_supported(arch: ArchSpec, scope) -> None:
    """Raises the scope's error unless its backward is built for `arch`; scope: a FitScope or its name.  The whole-layer scope without a decoder
    self-attention is a ValueError: there is nothing to fit."""
    s = FIT_SCOPES[scope] if isinstance(scope, str) else scope
    if s is FIT_LAYER and not arch.do_self_attn:
        raise ValueError("fit_scope=layer needs model.decoder_do_self_attn=True: without the self-attention the layer scope has nothing to fit "
                         "beyond fit_scope=cross")
    if not getattr(_lib.load(), s.supported)(*(getattr(arch, a) for a in s.supported_args)):
        raise s.error("the " + s.built_for.format(a=arch))


class U8Image:
    """One decoded image on the device with its input-stage geometry (cs_u8_image): data (h, w, 3) uint8 CUDA tensor (rows may be padded:
    row_bytes), rs = size after T.Resize, (crop_y, crop_x) = top-left corner of the processed window.  data None = the all-zero placeholder
    image the reference pads short reference lists with (nvs_dataset.py:459-470)."""
    __slots__ = ("data", "h", "w", "row_bytes", "rs", "crop_y", "crop_x")

    def __init__(self, data: Optional[torch.Tensor], h: int, w: int, rs, crop_y: int = 0, crop_x: int = 0, row_bytes: Optional[int] = None):
        if data is not None and (not data.is_cuda or data.dtype != torch.uint8 or not data.is_contiguous()):
            raise ValueError("U8Image.data must be a contiguous uint8 CUDA tensor")
        self.data, self.h, self.w, self.rs, self.crop_y, self.crop_x = data, int(h), int(w), (int(rs[0]), int(rs[1])), int(crop_y), int(crop_x)
        self.row_bytes = int(row_bytes) if row_bytes is not None else 3 * self.w

    def c_struct(self) -> "_lib.CsU8Image":
        return _lib.CsU8Image(C.c_void_p(self.data.data_ptr()) if self.data is not None else None, self.h, self.w, self.row_bytes,
                              self.rs[0], self.rs[1], self.crop_y, self.crop_x)


class U8Batch:
    """The images of a forward as decoded uint8 (what CrossScoreNet.forward and its siblings take in place of fp32 tensors): `images` in batch
    order (references item-major: item 0's N views, item 1's, ...), all producing the same (H, W) window; mean_std = the six T.Normalize numbers (task/predict.py:68-74).
    device: where the batch runs when every image is a placeholder (data None: nothing to take it from), e.g. zero_reference's reference keys."""

    def __init__(self, images, size, mean_std=synth.IMAGENET_MEAN_STD, device=None):
        self.images, self.size = list(images), (int(size[0]), int(size[1]))
        self.mean = (C.c_float * 3)(*mean_std[:3])
        self.std = (C.c_float * 3)(*mean_std[3:])
        self._device = torch.device(device) if device is not None else None

    def __len__(self) -> int:
        return len(self.images)

    def c_array(self, lo: int, hi: int):
        arr = (_lib.CsU8Image * (hi - lo))()
        for i in range(lo, hi):
            arr[i - lo] = self.images[i].c_struct()
        return arr

    def record_stream(self, s) -> None:
        for im in self.images:
            if im.data is not None:
                im.data.record_stream(s)

    @property
    def device(self):
        for im in self.images:
            if im.data is not None:
                return im.data.device
        return self._device


class SelectionBank:
    """What forward_select chooses from: tokens (R, h*w, C) in the module's operand type (encode_references of every candidate, contiguous),
    their descriptors mean / unit (R, C) and centre (C) fp32 (CrossScoreNet.reference_descriptors), and n_references, the views a query takes.
    A grouped bank also has `offsets` (G + 1 host integers: group g is the rows offsets[g] .. offsets[g + 1] - 1, the rows from offsets[G] on
    belong to no group), a centre per group (G, C), and `blank_row`: -1, or the row behind every group whose tokens stand in where a query's
    group is shorter than n_references (the encoder's tokens of the all-zero placeholder image)."""
    __slots__ = ("tokens", "mean", "centre", "unit", "n_references", "offsets", "blank_row", "row_place")

    def __init__(self, tokens: torch.Tensor, mean: torch.Tensor, centre: torch.Tensor, unit: torch.Tensor, n_references: int, offsets=None,
                 blank_row: int = -1):
        if tokens.dim() != 3 or not tokens.is_cuda or not tokens.is_contiguous():
            raise ValueError("SelectionBank.tokens must be a contiguous CUDA tensor (R, h*w, C)")
        R, _, Cc = tokens.shape
        if offsets is None:
            if int(blank_row) != -1:
                raise ValueError("SelectionBank.blank_row needs a grouped bank (offsets)")
            centre_shape = (Cc,)
        else:
            offsets = _group_offsets(offsets, R)
            centre_shape = (len(offsets) - 1, Cc)
            if not (int(blank_row) == -1 or int(offsets[-1]) <= int(blank_row) < R):
                raise ValueError(f"SelectionBank.blank_row = {blank_row} must be -1 or a row in [{int(offsets[-1])}, {R}), behind every group")
        for name, t, shape in (("mean", mean, (R, Cc)), ("centre", centre, centre_shape), ("unit", unit, (R, Cc))):
            if tuple(t.shape) != shape or t.dtype != torch.float32 or t.device != tokens.device or not t.is_contiguous():
                raise ValueError(f"SelectionBank.{name} must be a contiguous fp32 tensor {shape} on the tokens' device")
        self.tokens, self.mean, self.centre, self.unit, self.n_references = tokens, mean, centre, unit, int(n_references)
        self.offsets, self.blank_row = offsets, int(blank_row)
        # (R) int64 on the device: a row's place inside its group = its column of a query's similarities (0 for the rows behind the groups)
        self.row_place = None
        if offsets is not None:
            place = np.zeros(R, dtype=np.int64)
            for lo, hi in zip(offsets[:-1], offsets[1:]):
                place[lo:hi] = np.arange(hi - lo)
            self.row_place = torch.from_numpy(place).to(tokens.device)

    @property
    def longest_group(self) -> int:
        return int(len(self)) if self.offsets is None else int(np.diff(self.offsets).max())

    def __len__(self) -> int:
        return int(self.tokens.shape[0])


def _group_offsets(offsets, R: int) -> np.ndarray:
    """offsets of a grouped bank of R rows as a contiguous int32 array, checked: they start at 0, increase strictly and end inside the bank"""
    o = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64).reshape(-1))
    if o.size < 2 or o[0] != 0 or np.any(np.diff(o) <= 0) or o[-1] > R:
        raise ValueError(f"group offsets must start at 0, increase strictly and end inside the bank's {R} rows: {o.tolist()[:8]}{'...' if o.size > 8 else ''}")
    return o.astype(np.int32)


def _u8_form(*imgs) -> bool:
    """Whether a call's image arguments are U8Batch objects (else fp32 tensors): this picks the C entry point.  One call takes one form."""
    u8 = [isinstance(x, U8Batch) for x in imgs if x is not None]
    if any(u8) and not all(u8):
        raise ValueError("a call takes its images in one form: U8Batch objects or fp32 tensors, not both")
    return any(u8)


def _images(x, b0: int, b1: int, per_item: int = 1):
    """The C argument for the images of the items b0 .. b1 - 1 in either form (a U8Batch of references holds per_item images an item)."""
    return x.c_array(b0 * per_item, b1 * per_item) if isinstance(x, U8Batch) else C.c_void_p(x[b0:b1].data_ptr())


def _norm(x) -> tuple:
    """The (mean, std) pair a *_u8 entry point takes in front of its tail; the fp32 form is normalised already."""
    return (x.mean, x.std) if isinstance(x, U8Batch) else ()


class _Node(torch.nn.Module):
    """Parameter container; the tree of _Nodes reproduces the reference module paths."""


class CrossScoreNet(torch.nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        m = cfg.model
        # model.do_reference_cross=False (task/core.py:55,89): the reference builds no CrossReferenceNet (its state dict has no `ref_cross.*`
        # entries), runs the encoder for nothing and returns an EMPTY result dict.  Same here, minus the wasted encoder pass: the module keeps
        # the backbone / PE parameters so that such a checkpoint loads strictly, and forward() returns {} after the reference's own input checks.
        self._do_reference_cross = bool(m.do_reference_cross)
        # model/positional_encoding.py:61-69 hands the mode to F.interpolate together with align_corners=True, which torch accepts for a 4-D tensor
        # only with the interpolating modes bilinear and bicubic: every other value raises there ("align_corners option can only be set with
        # the interpolating modes ...") -- at the first forward whose patch grid differs from the PE's (pe_h, pe_w), not before: a grid that
        # matches adds the parameter as it is (positional_encoding.py:51-56) whatever the mode says.  Same here: `_check_pe_mode`.
        self._pe_mode_name = str(m.pos_enc.multi_view.interpolate_mode)
        self._pe_mode = {"bilinear": 0, "bicubic": 1}.get(self._pe_mode_name, 0)  # (an unsupported name never reaches the resize kernel)
        self.arch = arch_from_cfg(cfg)
        metric = m.predict.metric
        self._act, self._pow = regression_activation(metric.type, metric.min, metric.max, metric.power_factor)
        # parameter tree with the checkpoint's key names (all frozen for inference)
        for name, shape, kind, _ in synth.state_dict_spec(self.arch):
            if not self._do_reference_cross and name.startswith("ref_cross."):
                continue
            parts = name.split(".")
            node = self
            for p in parts[:-1]:
                if not hasattr(node, p):
                    node.add_module(p, _Node())
                node = getattr(node, p)
            if name == "img_mean_std":
                node.register_buffer(parts[-1], torch.tensor(synth.IMAGENET_MEAN_STD, dtype=torch.float32))
            else:
                node.register_parameter(parts[-1], torch.nn.Parameter(torch.zeros(shape, dtype=torch.float32), requires_grad=False))
        self._handle = None
        self._handle_device = None
        self._dirty = True
        self.enc_chunk_images = 0  # 0 = library default
        self.lanes = 0             # 0 = library default (2 concurrent lanes); 1 = serial
        # encoder position-embedding resize: "size" (installed transformers, the goldens) or "scale_factor" (the reference's pinned 4.33.3);
        # an optional key of THIS build under model.backbone (the reference has no such key): pos_embed_interpolation
        self._pos_legacy = str(cfg.model.backbone.get("pos_embed_interpolation", "size")) == "scale_factor"
        self.enc_fused = 0         # 0 = token-panel kernel per encoder layer where supported (hidden 384), 1 = unfused kernels
        self.ln_fold = 0           # 1 = fold the encoder LayerNorms into the QKV / fc1 GEMM epilogues (opt-in; slower so far)
        # 16-bit operand type of the MFMA kernels: "fp16" (default: 11 significant bits, finite to 65504) or "bf16" (8 bits, fp32's range:
        # the mode for checkpoints whose activations leave the half range; nonfinite_count() tells).  An optional key of THIS build:
        # model.backbone.operand_dtype; the predict driver derives it from the reference's own trainer.precision key.
        self.operand_dtype = str(cfg.model.backbone.get("operand_dtype", "fp16"))
        self._capture = False      # debug taps (debug_capture / debug_read): stage-level parity tests only
        self.finite_check = True   # every forward counts the non-finite values of its score map on the device (~3 us)
        self._after_sub_batch = None  # fit_head_step's / fit_tail_step's hook behind each sub-batch's forward call (_score)
        self._tail_keep = False    # fit_tail_keep: forwards keep what the tail's backward reads (fit_tail_step turns it on for its call)
        self._layer_keep = False   # fit_layer_keep: ... and what the self-attention block's backward reads (fit_layer_step, for its call)
        self._cross_keep = False   # fit_cross_keep: ... and what the cross-attention block's backward reads (fit_cross_step, for its call)
        self.register_load_state_dict_post_hook(lambda module, incompatible: module._mark_dirty())

    # -- weights ----------------------------------------------------------------------------------------------
    def _mark_dirty(self):
        self._dirty = True

    def _apply(self, fn, *args, **kwargs):
        # .to() / .cuda() / .half() / .bfloat16() replace the parameter tensors: the handle's packed copies are stale afterwards
        self._mark_dirty()
        return super()._apply(fn, *args, **kwargs)

    def load_numpy_state_dict(self, sd: Dict[str, np.ndarray]) -> None:
        self.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=True)

    def _operand_code(self) -> int:
        if self.operand_dtype not in ("fp16", "bf16"):
            raise ValueError(f"operand_dtype must be 'fp16' or 'bf16', got {self.operand_dtype!r}")
        return 1 if self.operand_dtype == "bf16" else 0

    @property
    def token_dtype(self) -> torch.dtype:
        """dtype of the cached reference tokens (encode_references / forward_cached): the handle's 16-bit operand type"""
        return torch.bfloat16 if self._operand_code() else torch.float16

    def nonfinite_count(self) -> int:
        """Non-finite values the score maps of this module's forwards held since the last call (waits for the last forward; resets the
        count).  With fp16 operands an activation beyond 65504 turns into inf upstream and reaches the score map as NaN: a count > 0
        says "run this checkpoint with operand_dtype = 'bf16'"."""
        if self._handle is None:
            return 0
        n = C.c_longlong(0)
        _lib.check(_lib.load().cs_nonfinite_count(self._handle, C.byref(n)))
        return int(n.value)

    def forward_stats(self) -> dict:
        """Launch census of this module's last forward (cs_forward_stats): {"launches": kernel launches, "host_enqueue_ms": wall time the call
        took on the calling thread, "kernels": {name: count}}."""
        if self._handle is None:
            return {"launches": 0, "host_enqueue_ms": 0.0, "kernels": {}}
        n, ms, buf = C.c_int(0), C.c_double(0.0), C.create_string_buffer(1024)
        _lib.check(_lib.load().cs_forward_stats(self._handle, C.byref(n), C.byref(ms), buf, 1024))
        kern = {k: int(v) for k, v in (kv.split("=") for kv in buf.value.decode().split() if "=" in kv)}
        return {"launches": int(n.value), "host_enqueue_ms": float(ms.value), "kernels": kern}

    def _check_pe_mode(self, H: int, W: int) -> None:
        """The reference's F.interpolate call (positional_encoding.py:61-69) only runs when the patch grid differs from the PE table's."""
        P = self.arch.patch
        if self._pe_mode_name not in ("bilinear", "bicubic") and (H // P, W // P) != (self.arch.pe_h, self.arch.pe_w):
            raise ValueError(f"model.pos_enc.multi_view.interpolate_mode={self._pe_mode_name!r}: align_corners option can only be "
                             "set with the interpolating modes: linear | bilinear | bicubic | trilinear (4-D input: bilinear | bicubic)")

    def _release(self):
        if self._handle is not None:
            _lib.load().cs_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def _ensure_handle(self, device: torch.device):
        if not self._do_reference_cross:
            raise ValueError("model.do_reference_cross=False: this module has no cross-reference predictor (task/core.py:55) -- nothing to score or cache")
        if self._handle is not None and not self._dirty and self._handle_device == device:
            return self._handle
        lib = _lib.load()
        self._release()
        a = self.arch
        m = self.cfg.model
        cc = _lib.CsConfig(hidden=a.hidden, enc_layers=a.enc_layers, enc_heads=a.enc_heads, mlp_ratio=a.mlp_ratio, patch=a.patch,
                           pos_grid=a.pos_grid, pe_h=a.pe_h, pe_w=a.pe_w, dec_layers=a.dec_layers, dec_heads=a.dec_heads,
                           do_self_attn=int(bool(m.decoder_do_self_attn)), do_short_cut=int(bool(m.decoder_do_short_cut)),
                           act=self._act, pow_p=self._pow, enc_chunk_images=int(self.enc_chunk_images), ln_fold=int(self.ln_fold),
                           lanes=int(self.lanes), pos_interp_legacy=int(self._pos_legacy), enc_fused=int(self.enc_fused),
                           operand_dtype=self._operand_code(), pe_interp_mode=int(self._pe_mode), skip_finite_check=int(not self.finite_check), swiglu=int(bool(a.swiglu)))
        with torch.cuda.device(device):
            h = lib.cs_create(C.byref(cc))
            if not h:
                msg = _lib.last_error()
                raise NotImplementedError(msg) if "not in" in msg else ValueError(msg)
            try:
                kinds = {torch.float32: _lib.DTYPE_F32, torch.float16: _lib.DTYPE_F16, torch.bfloat16: _lib.DTYPE_BF16}
                for name, t in self.state_dict().items():
                    t = t.detach()
                    t = (t if t.dtype in kinds else t.to(torch.float32)).contiguous()  # net.half() / net.bfloat16() modules load as they are
                    shape = (C.c_int64 * t.dim())(*t.shape)
                    _lib.check(lib.cs_set_weight_typed(h, name.encode(), C.c_void_p(t.data_ptr()), int(t.is_cuda), kinds[t.dtype], t.dim(), shape))
                _lib.check(lib.cs_finalize(h))
            except Exception:
                lib.cs_destroy(h)
                raise
        self._handle, self._handle_device, self._dirty = h, device, False
        if self._capture:
            _lib.check(lib.cs_debug_capture(h, 1))
        if self._tail_keep:
            _lib.check(lib.cs_fit_tail_keep(h, 1))
        if self._cross_keep:
            _lib.check(lib.cs_fit_cross_keep(h, 1))
        if self._layer_keep:
            _lib.check(lib.cs_fit_layer_keep(h, 1))
        return h

    # -- forward ----------------------------------------------------------------------------------------------
    def _alloc_outputs(self, B, N, H, W, dev, need_attn_weights, return_mean):
        """(score, attn, mean_out) of the four forward calls: the score map, and the attention map / per-image means when asked for."""
        P = self.arch.patch
        h, w = H // P, W // P
        score = torch.empty((B, h * P, w * P), dtype=torch.float32, device=dev)
        attn = torch.empty((B, h, w, N, h, w), dtype=torch.float32, device=dev) if need_attn_weights else None
        mean_out = torch.empty((B,), dtype=torch.float32, device=dev) if return_mean else None
        return score, attn, mean_out

    @staticmethod
    def _results(score, attn, mean_out):
        results = {"score_map_ref_cross": score, "attn_weights_map_ref_cross": attn}
        if mean_out is not None:
            results["score_mean_ref_cross"] = mean_out  # key does not start with "score_map": writers ignore it
        return results

    def _score(self, call, B, N, H, W, dev, need_attn_weights, head_id, return_mean, need_reference_use=False):
        """The plumbing every forward call shares: the outputs, the sub-batches (_sub_batches) and the result dict.  call(b0, b1, tail) makes
        the C call for the items b0 .. b1 - 1 and returns its code; tail = (score, attn | None, head id, mean | None, stream) of those items.
        need_reference_use arms cs_request_reference_use in front of every sub-batch's call, with that sub-batch's rows of the four outputs."""
        P = self.arch.patch
        with torch.cuda.device(dev):
            score, attn, mean_out = self._alloc_outputs(B, N, H, W, dev, need_attn_weights, return_mean)
            use = self._alloc_reference_use(B, N, H, W, dev) if need_reference_use else None
            stream = torch.cuda.current_stream(dev).cuda_stream
            for b0, b1 in self._sub_batches(B, N, (H // P) * (W // P)):
                if use is not None:
                    _lib.check(_lib.load().cs_request_reference_use(self._handle, *(C.c_void_p(t[b0:b1].data_ptr()) for t in use.values())))
                _lib.check(call(b0, b1, (C.c_void_p(score[b0:b1].data_ptr()), C.c_void_p(attn[b0:b1].data_ptr()) if attn is not None else None,
                                         int(head_id), C.c_void_p(mean_out[b0:b1].data_ptr()) if mean_out is not None else None,
                                         C.c_void_p(stream))))
                if self._after_sub_batch is not None:
                    self._after_sub_batch(b0, b1)  # fit_head_step: the head's backward over what this sub-batch's forward left behind
        results = self._results(score, attn, mean_out)
        if use is not None:
            results.update(use)
        return results

    def _alloc_reference_use(self, B, N, H, W, dev):
        """The four outputs of need_reference_use under their result keys, in cs_request_reference_use's argument order.
        None of the keys starts with "score_map": the writers iterate over that prefix."""
        h, w = H // self.arch.patch, W // self.arch.patch
        return {"ref_use_share": torch.empty((B, N, h, w), dtype=torch.float32, device=dev),
                "ref_use_peak_prob": torch.empty((B, N, h, w), dtype=torch.float32, device=dev),
                "ref_use_peak_index": torch.empty((B, N, h, w), dtype=torch.int32, device=dev),
                "ref_use_entropy": torch.empty((B, h, w), dtype=torch.float32, device=dev)}

    @torch.no_grad()
    def forward(self, query_img, ref_cross_imgs, need_attn_weights=False, need_attn_weights_head_id=0, norm_img=False,
                return_mean=False, need_reference_use=False):
        """
        :param need_reference_use: also return ref_use_share / ref_use_peak_prob / ref_use_peak_index (B, N, h, w) and ref_use_entropy (B, h, w):
                                which reference each query patch's last-layer cross-attention went to, where it looked, how spread it was
                                (mean over the heads).  Every forward* method takes it; the other outputs keep their bits.
        :param query_img:       (B, 3, H, W) fp32, ImageNet-normalised -- or a U8Batch of B decoded images
        :param ref_cross_imgs:  (B, N_ref_cross, 3, H, W) -- or a U8Batch of B * N images; one call takes one form
        :param norm_img:        reference flag (task/core.py:76-81), bug-for-bug: the std used is the mean.
        """
        u8 = _u8_form(query_img, ref_cross_imgs)
        if u8:
            # decoded uint8 images: query = B images, refs = B * N images (item-major).  The resize / crop / normalise of the input stage
            # happens inside the patch-embedding launch; results are bit-identical to InputStage + the fp32 form.
            if norm_img:
                raise ValueError("norm_img=True takes fp32 images: U8Batch inputs are normalised inside the patch-embedding launch")
            q, r, B = query_img, ref_cross_imgs, len(query_img)
            if B == 0 or len(r) % B or q.size != r.size:
                raise ValueError("expected B query images and B * N reference images of one processed size")
            N = len(r) // B
            H, W = q.size
            dev = q.device
            if dev is None:
                raise _lib.CrossScoreHipError("forward needs device images: the hot path has no CPU fallback")
        else:
            if not self._do_reference_cross:
                # task/core.py:84-117 with the flag off: features of the query (and of the references, when given) are computed and dropped, the
                # result dict stays empty.  The input checks of get_featmaps (:119-138: a 4-D query, references that concatenate with it) still hold.
                if query_img.dim() != 4 or query_img.shape[1] != 3:
                    raise ValueError("expected query_img (B,3,H,W)")
                if ref_cross_imgs is not None and (ref_cross_imgs.dim() != 5 or ref_cross_imgs.shape[0] != query_img.shape[0] or
                                                   tuple(ref_cross_imgs.shape[2:]) != tuple(query_img.shape[1:])):
                    raise ValueError("expected ref_cross_imgs (B,N,3,H,W) matching query_img")
                return {}
            if ref_cross_imgs is None:
                raise ValueError("ref_cross_imgs is required when model.do_reference_cross=True (task/core.py:90)")
            if query_img.dim() != 4 or query_img.shape[1] != 3 or ref_cross_imgs.dim() != 5 or ref_cross_imgs.shape[2] != 3:
                raise ValueError("expected query_img (B,3,H,W) and ref_cross_imgs (B,N,3,H,W)")
            if ref_cross_imgs.shape[0] != query_img.shape[0] or ref_cross_imgs.shape[-2:] != query_img.shape[-2:]:
                raise ValueError("query and reference batch / image sizes differ")
            if not query_img.is_cuda:
                raise _lib.CrossScoreHipError("CrossScoreNet.forward needs CUDA(HIP) tensors: the hot path has no CPU fallback")
            dev = query_img.device
            if norm_img:
                mean = self.img_mean_std.to(dev)[None, :3, None, None]
                query_img = (query_img - mean) / mean  # sic: task/core.py:77-79 divides by the mean
                ref_cross_imgs = (ref_cross_imgs - mean[:, None]) / mean[:, None]
            q = query_img.to(torch.float32).contiguous()
            r = ref_cross_imgs.to(device=dev, dtype=torch.float32).contiguous()
            B, _, H, W = q.shape
            N = r.shape[1]
        self._check_pe_mode(H, W)
        handle = self._ensure_handle(dev)
        fn = _lib.load().cs_forward_u8 if u8 else _lib.load().cs_forward
        return self._score(lambda b0, b1, tail: fn(handle, _images(q, b0, b1), _images(r, b0, b1, N), b1 - b0, N, H, W, *_norm(q), *tail),
                           B, N, H, W, dev, need_attn_weights, need_attn_weights_head_id, return_mean, need_reference_use)

    def _sub_batches(self, B: int, N: int, Np: int):
        """Items are independent, so a batch whose decoder buffers would overflow the kernels' 32-bit element offsets
        (B*N*Np*4C >= 2^31, e.g. ViT-B with 128 items) is scored in sub-batches; results are identical either way."""
        kv_per_item = N * Np * 2 * self.arch.hidden * self.arch.dec_layers
        step = max(1, min(B, (2 ** 31 - 1) // max(kv_per_item, 1)))
        return [(b0, min(B, b0 + step)) for b0 in range(0, B, step)]

    # -- reference-feature cache: a separate mode, bit-identical results ---------------------------
    @torch.no_grad()
    def encode_references(self, ref_imgs):
        """(R,3,H,W) normalised reference images, or a U8Batch of R decoded ones -> (R, h*w, C) fp16 decoder-ready tokens (final LN + multi-view
        PE).  A reference's tokens depend neither on the query nor on its view slot, so they can be computed once per image of
        reference_dir and gathered per query."""
        u8 = _u8_form(ref_imgs)
        if u8:
            x, R, (H, W), dev = ref_imgs, len(ref_imgs), ref_imgs.size, ref_imgs.device
            if R == 0 or dev is None:
                raise ValueError("expected at least one device image")
        else:
            if ref_imgs.dim() != 4 or ref_imgs.shape[1] != 3 or not ref_imgs.is_cuda:
                raise ValueError("expected CUDA ref_imgs (R,3,H,W)")
            dev = ref_imgs.device
            x = ref_imgs.to(torch.float32).contiguous()
            R, _, H, W = x.shape
        self._check_pe_mode(H, W)
        P = self.arch.patch
        handle = self._ensure_handle(dev)
        fn = _lib.load().cs_encode_references_u8 if u8 else _lib.load().cs_encode_references
        with torch.cuda.device(dev):
            tok = torch.empty((R, (H // P) * (W // P), self.arch.hidden), dtype=self.token_dtype, device=dev)
            _lib.check(fn(handle, _images(x, 0, R), R, H, W, *_norm(x), C.c_void_p(tok.data_ptr()),
                          C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        return tok

    @torch.no_grad()
    def forward_cached(self, query_img, ref_tokens, need_attn_weights=False, need_attn_weights_head_id=0, return_mean=False,
                       need_reference_use=False):
        """forward() with the reference views given as cached tokens (B, N, h*w, C) fp16 from encode_references."""
        u8 = _u8_form(query_img)
        if u8:
            q, B, (H, W), dev = query_img, len(query_img), query_img.size, ref_tokens.device
            if ref_tokens.dim() != 4 or ref_tokens.shape[0] != B or not ref_tokens.is_cuda or ref_tokens.dtype != self.token_dtype:
                raise ValueError("expected CUDA ref_tokens (B,N,h*w,C) of this module's operand type")
        else:
            if query_img.dim() != 4 or ref_tokens.dim() != 4 or ref_tokens.shape[0] != query_img.shape[0]:
                raise ValueError("expected query_img (B,3,H,W) and ref_tokens (B,N,h*w,C)")
            if not query_img.is_cuda or not ref_tokens.is_cuda or ref_tokens.device != query_img.device:
                raise _lib.CrossScoreHipError("forward_cached needs CUDA(HIP) tensors on one device: the hot path has no CPU fallback")
            dev = query_img.device
            q = query_img.to(torch.float32).contiguous()
            if ref_tokens.dtype != self.token_dtype:
                raise ValueError(f"ref_tokens are {ref_tokens.dtype}, this module's operand type is {self.token_dtype}: encode them with the same module")
            B, _, H, W = q.shape
        t = ref_tokens.contiguous()
        N = t.shape[1]
        P = self.arch.patch
        self._check_pe_mode(H, W)
        if t.shape[2] != (H // P) * (W // P) or t.shape[3] != self.arch.hidden:
            raise ValueError("ref_tokens do not match the query's patch grid / hidden size")
        handle = self._ensure_handle(dev)
        fn = _lib.load().cs_forward_cached_u8 if u8 else _lib.load().cs_forward_cached
        return self._score(lambda b0, b1, tail: fn(handle, _images(q, b0, b1), C.c_void_p(t[b0:b1].data_ptr()), b1 - b0, N, H, W, *_norm(q), *tail),
                           B, N, H, W, dev, need_attn_weights, need_attn_weights_head_id, return_mean, need_reference_use)

    def u8_input_supported(self, img: U8Image, size, device=None) -> bool:
        """Whether forward / encode_references / forward_cached take this image geometry as a U8Batch (else: InputStage + the fp32 form)."""
        dev = device or (img.data.device if img.data is not None else None)
        if dev is None or not self._do_reference_cross:
            return False
        st = img.c_struct()
        return bool(_lib.load().cs_u8_input_supported(self._ensure_handle(dev), C.byref(st), int(size[0]), int(size[1])))

    # -- reference selection by similarity: the choice of each query's views is made on the device ----------------------
    @torch.no_grad()
    def reference_descriptors(self, tokens, offsets=None):
        """(R, h*w, C) tokens from encode_references -> (mean (R, C), centre (C), unit (R, C)) fp32: the pooled descriptors of the candidates,
        their mean over the bank and the centred unit vectors forward_select compares a query's descriptor with.  With `offsets` (G + 1, see
        SelectionBank) every group has its own centre, (G, C), and the unit rows behind the last group are zeros."""
        if tokens.dim() != 3 or not tokens.is_cuda or tokens.dtype not in (torch.float16, torch.bfloat16):
            raise ValueError("expected CUDA tokens (R, h*w, C) in a 16-bit operand type")
        t = tokens.contiguous()
        R, Np, Cc = t.shape
        dev = t.device
        lib = _lib.load()
        with torch.cuda.device(dev):
            st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            grouped = offsets is not None
            off = _group_offsets(offsets, R) if grouped else None
            mean = torch.empty((R, Cc), dtype=torch.float32, device=dev)
            centre = torch.empty((len(off) - 1, Cc) if grouped else (Cc,), dtype=torch.float32, device=dev)
            unit = (torch.zeros if grouped else torch.empty)((R, Cc), dtype=torch.float32, device=dev)
            code = _lib.DTYPE_BF16 if t.dtype == torch.bfloat16 else _lib.DTYPE_F16
            for r0 in range(0, R, 32768):  # (an image's mean does not depend on the launch it is part of)
                r1 = min(R, r0 + 32768)
                _lib.check(lib.cs_op_token_descriptors(C.c_void_p(t[r0:r1].data_ptr()), r1 - r0, Np, Cc, code, C.c_void_p(mean[r0:r1].data_ptr()), st))
            if grouped:
                _lib.check(lib.cs_op_group_descriptors(C.c_void_p(mean.data_ptr()), R, Cc, off.ctypes.data_as(C.c_void_p), len(off) - 1,
                                                       C.c_void_p(centre.data_ptr()), C.c_void_p(unit.data_ptr()), st))
            else:
                _lib.check(lib.cs_op_descriptor_centre(C.c_void_p(mean.data_ptr()), R, Cc, C.c_void_p(centre.data_ptr()), st))
                _lib.check(lib.cs_op_descriptor_unit(C.c_void_p(mean.data_ptr()), R, Cc, C.c_void_p(centre.data_ptr()), C.c_void_p(unit.data_ptr()), st))
        return mean, centre, unit

    def _forward_select(self, query, bank, exclude, need_attn_weights, need_attn_weights_head_id, return_mean, n_references, group=None,
                        need_reference_use=False):
        u8 = _u8_form(query)
        N = int(bank.n_references if n_references is None else n_references)
        t = bank.tokens
        dev = t.device
        if t.dtype != self.token_dtype:
            raise ValueError(f"the bank's tokens are {t.dtype}, this module's operand type is {self.token_dtype}: encode them with the same module")
        if u8:
            q, B, (H, W) = query, len(query), query.size
            if B == 0:
                raise ValueError("expected at least one query image")
        else:
            if query.dim() != 4 or query.shape[1] != 3:
                raise ValueError("expected query_img (B,3,H,W)")
            if not query.is_cuda or query.device != dev:
                raise _lib.CrossScoreHipError("forward_select needs the query and the bank on one CUDA(HIP) device: the hot path has no CPU fallback")
            q = query.to(torch.float32).contiguous()
            B, _, H, W = q.shape
        P = self.arch.patch
        h, w = H // P, W // P
        R = len(bank)
        if t.shape[1] != h * w or t.shape[2] != self.arch.hidden:
            raise ValueError("the bank's tokens do not match the query's patch grid / hidden size")
        if N < 1:
            raise ValueError("forward_select needs at least one reference view per query")
        ex = None
        if exclude is not None:
            if tuple(exclude.shape) != (B,) or exclude.device != dev:
                raise ValueError("exclude must hold one bank index (or -1) per query, on the bank's device")
            ex = exclude.to(torch.int32).contiguous()
        grouped = bank.offsets is not None
        if grouped:
            if group is None:
                raise ValueError("a grouped bank needs `group`: the group each query chooses from")
            grp = np.ascontiguousarray(np.asarray(group.cpu() if isinstance(group, torch.Tensor) else group, dtype=np.int64).reshape(-1))
            if grp.shape != (B,) or np.any(grp < 0) or np.any(grp >= len(bank.offsets) - 1):
                raise ValueError(f"group must hold one group id in [0, {len(bank.offsets) - 1}) per query")
            grp = grp.astype(np.int32)
        elif group is not None:
            raise ValueError("`group` needs a grouped bank (SelectionBank with offsets)")
        self._check_pe_mode(H, W)
        lib = _lib.load()
        handle = self._ensure_handle(dev)
        fn = getattr(lib, "cs_forward_select" + ("_grouped" if grouped else "") + ("_u8" if u8 else ""))
        bank_args = (C.c_void_p(t.data_ptr()), C.c_void_p(bank.unit.data_ptr()), C.c_void_p(bank.centre.data_ptr()), R)
        with torch.cuda.device(dev):
            index = torch.empty((B, N), dtype=torch.int32, device=dev)
            sim = torch.empty((B, bank.longest_group), dtype=torch.float32, device=dev)

            def call(b0, b1, tail):
                # (a grouped bank's host arrays are copied into a pinned slot inside the call: they need not outlive it)
                groups = (bank.offsets.ctypes.data_as(C.c_void_p), len(bank.offsets) - 1, grp[b0:b1].ctypes.data_as(C.c_void_p),
                          bank.blank_row) if grouped else ()
                return fn(handle, _images(q, b0, b1), *bank_args, *groups,
                          C.c_void_p(ex[b0:b1].data_ptr()) if ex is not None else None, b1 - b0, N, H, W, *_norm(q),
                          *tail[:4], C.c_void_p(index[b0:b1].data_ptr()), C.c_void_p(sim[b0:b1].data_ptr()), tail[4])

            results = self._score(call, B, N, H, W, dev, need_attn_weights, need_attn_weights_head_id, return_mean, need_reference_use)
            results["reference_index"] = index
            # the similarities of the chosen entries, in the order chosen (an index of -1, a query that ran out of candidates, reads entry 0)
            if grouped:  # a column of sim is a place in the query's group; a padded place (-1) is NaN
                picked = torch.gather(sim, 1, bank.row_place[index.clamp(min=0).to(torch.int64)])
                results["reference_similarity"] = torch.where(index >= 0, picked, float("nan"))
            else:
                results["reference_similarity"] = torch.gather(sim, 1, index.clamp(min=0).to(torch.int64))
        return results

    @torch.no_grad()
    def forward_select(self, query_img, bank: "SelectionBank", exclude=None, need_attn_weights=False, need_attn_weights_head_id=0,
                       return_mean=False, n_references=None, group=None, need_reference_use=False):
        """forward_cached() with each query's N = bank.n_references views chosen on the device: the bank entries most similar to the query's own
        pooled descriptor, descending, ties to the lower index, exclude[b] (int32 (B), -1 = none) left out.  The result also holds
        "reference_index" (B, N) int32 and "reference_similarity" (B, N) fp32; the score map, mean and attention weights are bit-identical to
        forward_cached(query_img, bank.tokens[reference_index]).  query_img: fp32 (B, 3, H, W) or a U8Batch.  A grouped bank needs `group`, one
        group id per query (host integers): the query chooses among that group's rows only, a group shorter than N leaves -1 in reference_index and NaN in reference_similarity, and
        those places are fed bank.blank_row's tokens (zeros when it is -1)."""
        return self._forward_select(query_img, bank, exclude, need_attn_weights, need_attn_weights_head_id, return_mean, n_references, group, need_reference_use)

    def calibrate_lanes(self, query_img, ref_cross_imgs, tries: int = 3, steps: int = 4, min_gain: float = 0.08) -> Dict[str, Any]:
        """Checks that this module's multi-lane forward really overlaps its lanes, and repairs it if not.  The lanes' streams are probed
        when they are drawn (cs_forward), but streams that passed the probe can still end up on one hardware queue when other queues were
        created in between: the forward then silently runs 8.3-8.7 instead of 7.2 ms per cfg-2 batch.  This times `steps`
        forwards limited to one lane, then as configured; if the configured form does not win by `min_gain`, the lane streams are drawn
        again, up to `tries` times or until a set wins.  Call once with inputs of the working shape, outside any timed region.
        Returns what it measured.  Results of forwards are bit-identical whatever the lanes."""
        import time

        if self.lanes == 1:
            return {"one_lane_s": None, "lanes_s": []}
        lib = _lib.load()
        dev = query_img.device

        def run(n):
            for _ in range(n):
                self(query_img, ref_cross_imgs, False, 0, False)
            torch.cuda.synchronize(dev)

        def timed():
            run(1)
            t0 = time.perf_counter()
            run(steps)
            return (time.perf_counter() - t0) / steps

        run(2)  # handle, workspace, tables, lane streams exist from here on
        _lib.check(lib.cs_set_lanes(self._handle, 1))
        try:
            one = timed()
        finally:
            _lib.check(lib.cs_set_lanes(self._handle, 0))
        seen = []
        for attempt in range(max(1, tries)):
            if attempt:
                _lib.check(lib.cs_redraw_lane_streams(self._handle))
            seen.append(timed())
            if seen[-1] < (1.0 - min_gain) * one:
                break
        return {"one_lane_s": one, "lanes_s": seen}

    # -- fitting on the device: the scopes FIT_HEAD < FIT_TAIL < FIT_CROSS < FIT_LAYER of the table above --------
    HEAD_KEYS = FIT_HEAD.keys(0)  # (the head's keys name no layer)
    TAIL_KEYS = property(lambda self: FIT_TAIL.keys(self.arch.dec_layers), doc="the ten keys of the tail, in the order of cs_tail_backward's gradients")
    CROSS_KEYS = property(lambda self: FIT_CROSS.keys(self.arch.dec_layers), doc="the sixteen keys of the cross-attention fit, in cs_cross_backward's order")

    LAYER_KEYS = property(lambda self: FIT_LAYER.keys(self.arch.dec_layers), doc="the twenty-two keys of the whole-layer fit, in cs_layer_backward's order")

    def _fit_parameters(self, scope: FitScope):
        if not self._do_reference_cross:
            raise ValueError("model.do_reference_cross=False: this module has no regression head and no decoder to fit")
        return [self.get_parameter(k) for k in scope.keys(self.arch.dec_layers)]

    def _fit_supported(self, scope: FitScope) -> bool:
        return bool(getattr(_lib.load(), scope.supported)(*(getattr(self.arch, a) for a in scope.supported_args)))

    def _fit_keep(self, scope: FitScope, on: bool) -> None:
        setattr(self, f"_{scope.name}_keep", bool(on))
        if self._handle is not None:
            _lib.check(getattr(_lib.load(), scope.keep)(self._handle, int(bool(on))))

    def _fit_backward(self, scope: FitScope, gt, inv_count, accumulate, out):
        if self._handle is None:
            raise _lib.CrossScoreHipError(f"{scope.name}_backward before any forward")
        dev = self._handle_device
        if gt.dim() != 3 or gt.dtype != torch.float32 or gt.device != dev or not gt.is_contiguous():
            raise ValueError("expected a contiguous fp32 gt (B, H, W) on the module's device")
        B, H, W = gt.shape
        if out is None:
            out = tuple(torch.zeros(p.shape, device=dev) for p in self._fit_parameters(scope)) + (torch.zeros((), dtype=torch.float64, device=dev),)
        inv = 1.0 / gt.numel() if inv_count is None else float(inv_count)
        with torch.cuda.device(dev):
            _lib.check(getattr(_lib.load(), scope.backward)(self._handle, C.c_void_p(gt.data_ptr()), B, H, W, inv, int(bool(accumulate)),
                                                            *(C.c_void_p(t.data_ptr()) for t in out),
                                                            C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        return out

    def _fit_step(self, scope: FitScope, query, refs, gt, state: "HeadFitState", ref_tokens):
        """One AdamW step of the scope's tensors on one batch: the forward through the existing path (forward, in either form of its images;
        forward_cached with ref_tokens) with the scope's keep switch on for the call, the scope's backward behind each sub-batch, cs_op_adamw on
        every tensor in place, then each scope of the chain hands its own tensors back (cs_set_*_weights).  The module is not marked dirty: the
        handle keeps every other packed weight.  gt: (B, h P, w P) fp32 on the device, the score map's shape.  Returns the loss of the batch
        BEFORE the step as a device fp64 scalar; nothing is waited for."""
        name = f"fit_{scope.name}_step"
        if (refs is None) == (ref_tokens is None):
            raise ValueError(f"{name} takes the references either as images (refs) or as cached tokens (ref_tokens)")
        check_fit_supported(self.arch, scope)
        params = self._fit_parameters(scope)
        dev = gt.device
        for p in params:
            if not p.is_cuda or p.device != dev or p.dtype != torch.float32 or not p.is_contiguous():
                raise ValueError(f"{name} needs the module's fp32 parameters on the device of the batch (net.to(device))")
        if gt.dim() != 3 or gt.dtype != torch.float32 or not gt.is_contiguous():
            raise ValueError("expected a contiguous fp32 gt (B, h P, w P)")
        state.prepare(params)
        lib = _lib.load()
        inv = 1.0 / gt.numel()
        grads, loss = state.grads, torch.zeros((), dtype=torch.float64, device=dev)
        H, W = gt.shape[1:]
        c_backward = getattr(lib, scope.backward)

        def backward(b0, b1):
            _lib.check(c_backward(self._handle, C.c_void_p(gt[b0:b1].data_ptr()), b1 - b0, H, W, inv, int(b0 > 0),
                                  *(C.c_void_p(g.data_ptr()) for g in grads), C.c_void_p(loss.data_ptr()),
                                  C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))

        kept = getattr(self, f"_{scope.name}_keep") if scope.keep else None
        self._after_sub_batch = backward
        try:
            if scope.keep:
                self._ensure_handle(dev)  # (the forward below finds it ready: the switch goes onto the handle it will use)
                self._fit_keep(scope, True)
            res = self.forward_cached(query, ref_tokens) if ref_tokens is not None else self.forward(query, refs)
        finally:
            self._after_sub_batch = None
            if scope.keep:
                self._fit_keep(scope, kept)
        if tuple(res["score_map_ref_cross"].shape) != tuple(gt.shape):
            raise ValueError(f"gt {tuple(gt.shape)} does not have the score map's shape {tuple(res['score_map_ref_cross'].shape)}")
        state.step += 1
        with torch.cuda.device(dev):
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            for p, m, v, g in zip(params, state.m, state.v, grads):
                _lib.check(lib.cs_op_adamw(C.c_void_p(p.data_ptr()), C.c_void_p(m.data_ptr()), C.c_void_p(v.data_ptr()), C.c_void_p(g.data_ptr()),
                                           p.numel(), state.lr, state.betas[0], state.betas[1], state.eps, state.weight_decay, state.step, None,
                                           stream))
            at = 0
            for s in scope.chain():  # cross, tail, head: each its own tensors
                own = params[at:at + len(s.own)]
                _lib.check(getattr(lib, s.set_weights)(self._handle, *(C.c_void_p(p.data_ptr()) for p in own), stream))
                at += len(own)
        return loss

    def head_parameters(self):
        """The four tensors of the regression head: head.0 weight (C, C) and bias (C), head.2 weight (P P, C) and bias (P P)."""
        return self._fit_parameters(FIT_HEAD)

    def tail_parameters(self):
        """The last decoder layer's linear1, linear2 and norm3, then the head: ten tensors in TAIL_KEYS order."""
        return self._fit_parameters(FIT_TAIL)

    def cross_parameters(self):
        """The last decoder layer's multihead_attn in_proj and out_proj and norm2, then the tail: sixteen tensors in CROSS_KEYS order."""
        return self._fit_parameters(FIT_CROSS)

    def layer_parameters(self):
        """The last decoder layer's self_attn in_proj and out_proj and norm1, then the cross-attention fit's: twenty-two tensors in LAYER_KEYS order."""
        return self._fit_parameters(FIT_LAYER)

    def head_fit_supported(self) -> bool:
        return self._fit_supported(FIT_HEAD)

    def tail_fit_supported(self) -> bool:
        return self._fit_supported(FIT_TAIL)

    def cross_fit_supported(self) -> bool:
        return self._fit_supported(FIT_CROSS)

    def layer_fit_supported(self) -> bool:
        return self._fit_supported(FIT_LAYER)

    def fit_layer_keep(self, on: bool = True) -> None:
        """Following forwards also keep what layer_backward reads (cs_fit_layer_keep): fit_cross_keep's copies, x0, and the last
        self-attention's output and lse."""
        self._fit_keep(FIT_LAYER, on)

    def fit_tail_keep(self, on: bool = True) -> None:
        """Following forwards also keep the last decoder layer's norm2 output and ReLU rows (cs_fit_tail_keep): what tail_backward reads."""
        self._fit_keep(FIT_TAIL, on)

    def fit_cross_keep(self, on: bool = True) -> None:
        """Following forwards also keep what cross_backward reads (cs_fit_cross_keep): fit_tail_keep's two copies, x1 and the last
        cross-attention's lse."""
        self._fit_keep(FIT_CROSS, on)

    def head_backward(self, gt, inv_count=None, accumulate=False, out=None):
        """cs_head_backward over the LAST forward call of this module (its last sub-batch): gt (B, h P, w P) fp32 on the device ->
        (dWa, dba, dWb, dbb, loss): fp32 gradients and the fp64 device scalar loss, each scaled by inv_count (default 1 / gt.numel())."""
        return self._fit_backward(FIT_HEAD, gt, inv_count, accumulate, out)

    def tail_backward(self, gt, inv_count=None, accumulate=False, out=None):
        """The same through cs_tail_backward (that forward run with fit_tail_keep on): the ten gradients in TAIL_KEYS order and the loss."""
        return self._fit_backward(FIT_TAIL, gt, inv_count, accumulate, out)

    def cross_backward(self, gt, inv_count=None, accumulate=False, out=None):
        """The same through cs_cross_backward (that forward run with fit_cross_keep on): the sixteen gradients in CROSS_KEYS order and the loss."""
        return self._fit_backward(FIT_CROSS, gt, inv_count, accumulate, out)

    def layer_backward(self, gt, inv_count=None, accumulate=False, out=None):
        """The same through cs_layer_backward (that forward run with fit_layer_keep on): the twenty-two gradients in LAYER_KEYS order and the loss."""
        return self._fit_backward(FIT_LAYER, gt, inv_count, accumulate, out)

    def fit_head_step(self, query, refs, gt, state: "HeadFitState", ref_tokens=None):
        """_fit_step over the four tensors of the head: cs_head_backward, four cs_op_adamw launches, cs_set_head_weights."""
        return self._fit_step(FIT_HEAD, query, refs, gt, state, ref_tokens)

    def fit_tail_step(self, query, refs, gt, state: "HeadFitState", ref_tokens=None):
        """_fit_step over the ten tensors of the tail: cs_tail_backward on a forward with fit_tail_keep on, cs_set_tail_weights and the head's."""
        return self._fit_step(FIT_TAIL, query, refs, gt, state, ref_tokens)

    def fit_cross_step(self, query, refs, gt, state: "HeadFitState", ref_tokens=None):
        """_fit_step over the sixteen tensors of the cross-attention fit: cs_cross_backward on a forward with fit_cross_keep on,
        cs_set_cross_weights, the tail's and the head's."""
        return self._fit_step(FIT_CROSS, query, refs, gt, state, ref_tokens)

    def fit_layer_step(self, query, refs, gt, state: "HeadFitState", ref_tokens=None):
        """_fit_step over the twenty-two tensors of the whole-layer fit: cs_layer_backward on a forward with fit_layer_keep on,
        cs_set_layer_weights, the cross-attention fit's, the tail's and the head's."""
        return self._fit_step(FIT_LAYER, query, refs, gt, state, ref_tokens)

    def _debug_inputs(self, c_name: str, rows: int, specs):
        """Fresh tensors of specs' (shape, dtype) filled by the library's cs_debug_*_inputs `c_name` from the last forward call; rows = its B h w,
        checked by the library (tests)."""
        if self._handle is None:
            raise _lib.CrossScoreHipError(f"{c_name[len('cs_debug_'):]} before any forward")
        dev = self._handle_device
        with torch.cuda.device(dev):
            out = tuple(torch.empty(shape, dtype=dtype, device=dev) for shape, dtype in specs)
            _lib.check(getattr(_lib.load(), c_name)(self._handle, *(C.c_void_p(t.data_ptr()) for t in out), int(rows),
                                                    C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        return out

    def head_inputs(self, rows: int):
        """(X, A): the 16-bit tokens behind the last norm3 and the head's hidden rows of the last forward call, (rows, C) each."""
        rc = (int(rows), self.arch.hidden)
        return self._debug_inputs("cs_debug_head_inputs", rows, [(rc, self.token_dtype)] * 2)

    def tail_inputs(self, rows: int):
        """(x2, H): the fp32 output of the last layer's norm2 and the 16-bit rows relu(linear1(x2)) of the last forward call, (rows, C) each;
        that forward must have run with fit_tail_keep on."""
        rc = (int(rows), self.arch.hidden)
        return self._debug_inputs("cs_debug_tail_inputs", rows, [(rc, torch.float32), (rc, self.token_dtype)])

    def cross_inputs(self, rows: int, N: int):
        """(x1, Q', O, lse, K, V) of the last forward call's last cross-attention: x1 (rows, C) fp32, Q' and O (rows, C) 16 bit, lse (rows heads)
        fp32 in (B, heads, Np) order, K and V (rows N, C) 16 bit; that forward must have run with fit_cross_keep on."""
        Cc, t16 = self.arch.hidden, self.token_dtype
        rc, kv = (int(rows), Cc), (int(rows) * int(N), Cc)
        return self._debug_inputs("cs_debug_cross_inputs", rows, [(rc, torch.float32), (rc, t16), (rc, t16),
                                                                  ((int(rows) * self.arch.dec_heads,), torch.float32), (kv, t16), (kv, t16)])

    def layer_inputs(self, rows: int):
        """(x0, Qs', Ks, Vs, Os, lse_s) of the last forward call's last self-attention: x0 (rows, C) fp32, the three blocks of the packed projection
        and Os (rows, C) 16 bit, lse_s (rows heads) fp32 in (B, heads, Np) order; that forward must have run with fit_layer_keep on."""
        rc, t16 = (int(rows), self.arch.hidden), self.token_dtype
        return self._debug_inputs("cs_debug_layer_inputs", rows, [(rc, torch.float32), (rc, t16), (rc, t16), (rc, t16), (rc, t16),
                                                                  ((int(rows) * self.arch.dec_heads,), torch.float32)])

    # -- debug taps used by the stage-level parity tests (tests/test_hip_stages.py) ------------------------------------
    def debug_capture(self, on: bool = True) -> None:
        """Following forwards also keep their intermediate tensors (cs_debug_capture): not for timed runs."""
        self._capture = bool(on)
        if self._handle is not None:
            _lib.check(_lib.load().cs_debug_capture(self._handle, int(self._capture)))

    def debug_read(self, name: str) -> torch.Tensor:
        """Tap `name` of the last captured forward (include/crossscore_hip.h lists the names), in its own dtype and shape."""
        if self._handle is None:
            raise _lib.CrossScoreHipError("debug_read before any forward")
        lib = _lib.load()
        dt, nd, shp = C.c_int(), C.c_int(), (C.c_int64 * 4)()
        stream = C.c_void_p(torch.cuda.current_stream(self._handle_device).cuda_stream)
        _lib.check(lib.cs_debug_read(self._handle, name.encode(), None, 0, C.byref(dt), C.byref(nd), shp, stream))
        dtype = {_lib.DTYPE_F32: torch.float32, _lib.DTYPE_F16: torch.float16, _lib.DTYPE_BF16: torch.bfloat16}[dt.value]
        out = torch.empty(tuple(int(shp[k]) for k in range(nd.value)), dtype=dtype, device=self._handle_device)
        with torch.cuda.device(self._handle_device):
            _lib.check(lib.cs_debug_read(self._handle, name.encode(), C.c_void_p(out.data_ptr()), out.numel() * out.element_size(),
                                         C.byref(dt), C.byref(nd), shp, stream))
        return out

    # -- profiling hooks used by bench.py --------------------------------------------------------------------
    def profile_enable(self, on: bool) -> None:
        _lib.check(_lib.load().cs_profile_enable(self._handle, int(on)))

    def profile_read(self, family: int):
        ms, n, fl = C.c_double(), C.c_int(), C.c_double()
        _lib.check(_lib.load().cs_profile_read(self._handle, family, C.byref(ms), C.byref(n), C.byref(fl)))
        return ms.value, n.value, fl.value

    def profile_read_bytes(self, family: int) -> float:
        b = C.c_double()
        _lib.check(_lib.load().cs_profile_read_bytes(self._handle, family, C.byref(b)))
        return b.value


def load_lightning_checkpoint(path: str) -> Dict[str, torch.Tensor]:
    """`state_dict` of a CrossScore Lightning checkpoint with the "model." prefix removed
    (CrossScoreLightningModule.model = CrossScoreNet, task/core.py:173).  Optimizer / scheduler / callback
    state is ignored."""
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    sd = ckpt["state_dict"] if "state_dict" in ckpt else ckpt
    return {k[len("model."):]: v for k, v in sd.items() if k.startswith("model.")} or dict(sd)


class HeadFitState:
    """What fit_head_step, fit_tail_step, fit_cross_step or fit_layer_step keeps between steps: AdamW's moments of the scope's parameters, the step count (from 1
    at the first step), the learning rate (the driver's StepLR writes it) and the gradient buffers.  Defaults are torch.optim.AdamW's."""

    def __init__(self, lr: float = 5e-4, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2):
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.step = 0
        self.m = self.v = self.grads = None

    def prepare(self, params) -> None:
        if self.m is None or any(m.device != p.device for m, p in zip(self.m, params)):
            self.m = [torch.zeros_like(p, requires_grad=False) for p in params]
            self.v = [torch.zeros_like(p, requires_grad=False) for p in params]
            self.grads = [torch.zeros_like(p, requires_grad=False) for p in params]


def save_lightning_checkpoint(path: str, net: CrossScoreNet) -> None:
    """The module's state dict in the layout load_lightning_checkpoint (and the reference's Lightning module) reads: {"state_dict":
    {"model." + key: tensor}}, tensors on the CPU.  Optimiser state is not written."""
    sd = {"model." + k: v.detach().to("cpu").clone() for k, v in net.state_dict().items()}
    torch.save({"state_dict": sd}, path)
