"""Output side of the predict drop-in: what the reference writes after each batch and at the end of the run.

Mirrors
  BatchWriter                                   utils/io/batch_writer.py:26-135,155-270 (score maps, query / reference images, item-path
                                                json, attention-weight images of the centre query patch; ground-truth score maps in the
                                                test phase only, batch_writer.py:137-152)
  attn2rgb                                      utils/misc/image.py:55-77
  get_vrange / metric_map_write / gray2rgb      batch_writer.py:9-21, utils/io/images.py:49-63, utils/misc/image.py:37-52
  SummaryWriterPredictedOnlineTestPrediction    utils/io/score_summariser.py:142-250 (per-image mean -> CSV, "%.4f")
The float -> integer image conversion runs on the GPU (cs_op_score_to_gray16 / cs_op_score_to_rgb: 2 or 3 bytes per pixel cross
PCIe instead of 4).  PNG compression has two forms, chosen by `this_main.png_encoder`:
  host (default)   PIL's, on a thread pool, as in the reference (imageio); the processed query / reference images are de-normalised on the host
  gpu              cs_op_png_encode: score maps and processed images are converted (cs_op_score_to_*, cs_op_denorm_to_rgb8) and compressed on
                   the device, queued behind the forward; finished files cross PCIe into pinned memory and the pool threads only write them.
                   Pixel-exact, valid PNGs, not byte-equal to PIL's (independent 16-KiB segments).  `this_main.png_compression`: fast =
                   Sub filter, fixed-Huffman / stored blocks (larger files); compact = per-row adaptive filter, dynamic-Huffman blocks.
Attention-weight images and the item-path JSON always take the host path.  The reference-use images (this_main.reference_use_images; DESIGN.md 6,
f12) are coloured on the device for both encoders (cs_op_score_to_rgb on [0, 1]) and then take the chosen one, so the two give equal pixels.  The composite "vis" figure (task/core.py:422-434) has a form of this build's own, the preview sheet
of vis.py (this_main.vis_sheet), composed on the device from the integer images formed here.
"""
from __future__ import annotations

import csv
import ctypes as C
import json
import os
import threading
from pathlib import Path
from typing import Dict, List, Sequence

import numpy as np
import torch

from . import _lib
from .config import this_main_choice


def get_vrange(metric_type: str, metric_min: float, metric_max: float):
    """batch_writer.py:9-21: gray PNGs use the metric's intrinsic range, RGB the model's prediction range."""
    if metric_type == "ssim":
        intrinsic = [-1, 1]
    elif metric_type in ("mse", "mae"):
        intrinsic = [0, 1]
    else:
        raise ValueError(f"metric_type {metric_type} not supported")
    return intrinsic, [metric_min, metric_max]


def colormap_table(name: str = "turbo") -> np.ndarray:
    """(256, 3) uint8: u8() of the colormap's 256 entries (utils/misc/image.py:45-52, utils/io/images.py:20-23)."""
    import matplotlib

    lut = np.asarray(matplotlib.colormaps[name](np.arange(256)))[:, :3]
    return (lut * 255.0).astype(np.uint8)


def attn2rgb(attn_map: np.ndarray, table: np.ndarray) -> np.ndarray:
    """utils/misc/image.py:55-77: softmax weights on a log scale (eps = 1e-8) through the colormap; (H, W) fp32 -> (H, W, 3) uint8."""
    eps = 1e-8
    a = np.asarray(attn_map, np.float32).clip(0, 1)
    a = (a + eps).clip(0, 1)
    a = np.log(a) - np.log(eps)
    x = (a - 0.0) / np.float32(-np.log(eps) - 0.0)   # plt.Normalize(vmin=0, vmax=-log(eps)) on a float32 array
    x = x * np.float32(256)
    idx = x.astype(np.int64)
    idx[x == 256] = 255
    idx[~(x >= 0)] = 0
    idx[x > 256] = 255
    return table[np.clip(idx, 0, 255)]


def focus_map(entropy: torch.Tensor, n_ref: int) -> torch.Tensor:
    """entropy (B, h, w) in bits of an attention over n_ref * h * w keys -> 1 - entropy / log2(n_ref h w) in fp32: 1 where a patch looked at one
    key, 0 where it spread evenly over all of them.  (Formed as 1 - entropy * fp32(1 / log2(..)): two roundings, the same on host and device.)"""
    bits = float(np.log2(float(n_ref * entropy.shape[-2] * entropy.shape[-1])))
    if not bits > 0:
        return torch.ones_like(entropy, dtype=torch.float32)
    return 1.0 - entropy.float() * float(np.float32(1.0 / bits))


def unit_to_rgb8(values: torch.Tensor, lut: torch.Tensor) -> torch.Tensor:
    """(I, H, W) fp32 CUDA values -> (I, H, W, 3) uint8 through the 256-entry table `lut` on [0, 1] (cs_op_score_to_rgb: index trunc(256 x),
    below 0 the first entry, from 1 on the last)"""
    values = values.contiguous()
    out = torch.empty(tuple(values.shape) + (3,), dtype=torch.uint8, device=values.device)
    _lib.check(_lib.load().cs_op_score_to_rgb(C.c_void_p(values.data_ptr()), values.numel(), 0.0, 1.0, C.c_void_p(lut.data_ptr()), C.c_void_p(out.data_ptr()),
                                              C.c_void_p(torch.cuda.current_stream(values.device).cuda_stream)))
    return out


def name_stem(path: str) -> str:
    """batch_writer.py:112-115: last five path components joined by "_", ".png" removed."""
    return str(Path(*Path(path).parts[-5:])).replace("/", "_").replace(".png", "")


class ScoreMapEncoder:
    """Device score maps (B, H, W) fp32 -> host integer images, converted on the GPU."""

    def __init__(self, metric_type: str, metric_min: float, metric_max: float, colour_mode: str, device: torch.device):
        if colour_mode not in ("gray", "rgb"):
            raise ValueError(f"colour_mode {colour_mode} not supported")
        self.intrinsic, self.vis = get_vrange(metric_type, metric_min, metric_max)
        self.colour_mode = colour_mode
        self.device = device
        self._lut = torch.from_numpy(colormap_table("turbo").reshape(-1)).to(device) if colour_mode == "rgb" else None

    def device_image(self, score: torch.Tensor) -> torch.Tensor:
        """The integer image on the device: (B, H, W) int16 (16-bit samples, unsigned in memory) or (B, H, W, 3) uint8."""
        lib = _lib.load()
        score = score.contiguous()
        if score.dtype != torch.float32 or not score.is_cuda:
            raise ValueError("score maps must be fp32 CUDA tensors")
        n = score.numel()
        st = C.c_void_p(torch.cuda.current_stream(score.device).cuda_stream)
        if self.colour_mode == "gray":
            out = torch.empty(score.shape, dtype=torch.int16, device=score.device)  # 16-bit samples (viewed unsigned on the host)
            _lib.check(lib.cs_op_score_to_gray16(C.c_void_p(score.data_ptr()), n, 1 if self.intrinsic == [-1, 1] else 0, C.c_void_p(out.data_ptr()), st))
            return out
        out = torch.empty(tuple(score.shape) + (3,), dtype=torch.uint8, device=score.device)
        _lib.check(lib.cs_op_score_to_rgb(C.c_void_p(score.data_ptr()), n, float(self.vis[0]), float(self.vis[1]), C.c_void_p(self._lut.data_ptr()),
                                         C.c_void_p(out.data_ptr()), st))
        return out

    def __call__(self, score: torch.Tensor) -> np.ndarray:
        out = self.device_image(score).cpu().numpy()
        return out.view(np.uint16) if self.colour_mode == "gray" else out


class PngHandle:
    """Files of one asynchronous cs_op_png_encode call: bytes(i) waits for the call's event, then cuts file i out of the pinned block."""

    def __init__(self, event, host_out: torch.Tensor, host_len: torch.Tensor):
        self._event, self._out, self._len = event, host_out, host_len
        self._lock = threading.Lock()
        self._arr = None

    def __len__(self) -> int:
        return int(self._len.shape[0])

    def bytes(self, i: int) -> bytes:
        with self._lock:
            if self._arr is None:
                self._event.synchronize()
                self._arr = (self._out.numpy(), self._len.numpy())
        out, ln = self._arr
        if int(ln[i]) <= 0:  # the device's sign of a file that did not fit its slot (cs_png_bound would be wrong)
            raise RuntimeError(f"cs_op_png_encode produced no file for image {i}")
        return out[i, : int(ln[i])].tobytes()

    def result(self) -> List[bytes]:
        return [self.bytes(i) for i in range(len(self))]


PNG_COMPRESSIONS = {"fast": 0, "compact": _lib.PNG_DYNAMIC | _lib.PNG_ADAPTIVE_FILTER}  # cs_op_png_encode_ex flags


class PngEncoder:
    """Device integer images -> PNG files, compressed on the device (cs_op_png_encode_ex).  (I, H, W) int16 / uint16 tensors become 16-bit
    grayscale files, (I, H, W, 3) uint8 tensors 8-bit RGB files; pixel-exact, not byte-equal to PIL's.  compression: "fast" (Sub filter,
    fixed-Huffman / stored blocks: the bytes of cs_op_png_encode) or "compact" (per-row adaptive filter, dynamic-Huffman blocks: smaller
    files, more device time)."""

    def __init__(self, compression: str = "fast"):
        if compression not in PNG_COMPRESSIONS:
            raise ValueError(f"PngEncoder: compression {compression!r} not supported: fast | compact")
        self.compression = compression
        self.flags = PNG_COMPRESSIONS[compression]

    @staticmethod
    def _kind(pixels: torch.Tensor):
        if not pixels.is_cuda:
            raise ValueError("PngEncoder takes CUDA tensors")
        if pixels.dim() == 3 and pixels.dtype in (torch.int16, getattr(torch, "uint16", torch.int16)):
            return _lib.PNG_GRAY16, 2
        if pixels.dim() == 4 and pixels.shape[-1] == 3 and pixels.dtype == torch.uint8:
            return _lib.PNG_RGB8, 3
        raise ValueError(f"PngEncoder takes (I, H, W) 16-bit or (I, H, W, 3) uint8 tensors, not {tuple(pixels.shape)} {pixels.dtype}")

    def encode_async(self, pixels: torch.Tensor) -> PngHandle:
        """Queues the encode and the copy to pinned memory on the current stream; returns without waiting for either."""
        lib = _lib.load()
        kind, bpp = self._kind(pixels)
        pixels = pixels.contiguous()
        I, H, W = (int(v) for v in pixels.shape[:3])
        if I <= 0 or H <= 0 or W <= 0:
            raise ValueError(f"PngEncoder: empty batch or image {tuple(pixels.shape)}")
        dev = pixels.device
        slot = int(lib.cs_png_bound(kind, H, W))
        if slot == 0:
            raise NotImplementedError(f"PngEncoder: {H} x {W} images are larger than the encoder takes (4096 x 4096)")
        slot = (slot + 63) // 64 * 64
        out = torch.empty((I, slot), dtype=torch.uint8, device=dev)
        lengths = torch.empty((I,), dtype=torch.int32, device=dev)
        work = torch.empty((int(lib.cs_png_workspace_bytes(kind, I, H, W)),), dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream(dev)
        _lib.check(lib.cs_op_png_encode_ex(C.c_void_p(pixels.data_ptr()), kind, I, H, W, H * W * bpp, C.c_void_p(out.data_ptr()), slot,
                                           C.c_void_p(lengths.data_ptr()), C.c_void_p(work.data_ptr()), C.c_void_p(st.cuda_stream), self.flags))
        host_out = torch.empty((I, slot), dtype=torch.uint8, pin_memory=True)
        host_len = torch.empty((I,), dtype=torch.int32, pin_memory=True)
        host_out.copy_(out, non_blocking=True)
        host_len.copy_(lengths, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(st)
        return PngHandle(ev, host_out, host_len)

    def encode(self, pixels: torch.Tensor) -> List[bytes]:
        return self.encode_async(pixels).result()


def denorm_to_rgb8(imgs: torch.Tensor, img_mean_std: torch.Tensor) -> torch.Tensor:
    """cs_op_denorm_to_rgb8: (I, 3, H, W) fp32 processed images on the device -> (I, H, W, 3) uint8, BatchWriter._de_norm_u8 bit for bit."""
    lib = _lib.load()
    imgs = imgs.detach().contiguous()
    if imgs.dtype != torch.float32 or not imgs.is_cuda or imgs.dim() != 4 or imgs.shape[1] != 3:
        raise ValueError("denorm_to_rgb8 takes (I, 3, H, W) fp32 CUDA tensors")
    I, _, H, W = (int(v) for v in imgs.shape)
    ms = [float(v) for v in img_mean_std.detach().float().cpu().tolist()]
    mean, std = (C.c_float * 3)(*ms[:3]), (C.c_float * 3)(*ms[3:])
    out = torch.empty((I, H, W, 3), dtype=torch.uint8, device=imgs.device)
    _lib.check(lib.cs_op_denorm_to_rgb8(C.c_void_p(imgs.data_ptr()), I, H, W, mean, std, C.c_void_p(out.data_ptr()),
                                        C.c_void_p(torch.cuda.current_stream(imgs.device).cuda_stream)))
    return out


PNG_ENCODERS = ("host", "gpu")


def png_encoder_choice(cfg) -> str:
    """this_main.png_encoder (this build's key): host (default) | gpu."""
    return this_main_choice(cfg, "png_encoder", PNG_ENCODERS)


def png_compression_choice(cfg) -> str:
    """this_main.png_compression (this build's key): fast (default) | compact.  Takes effect with png_encoder=gpu only; ignored with host."""
    return this_main_choice(cfg, "png_compression", tuple(PNG_COMPRESSIONS))


def save_png(path, arr: np.ndarray) -> None:
    from PIL import Image

    # uint16 arrays become 16-bit grayscale PNGs ("I;16"): what imageio writes for the reference's int32 maps (utils/io/images.py:31-36)
    Image.fromarray(arr).save(path)


def save_png_bytes(path, handle: PngHandle, i: int) -> None:
    data = handle.bytes(i)  # waits for the encode's event in the pool thread
    with open(path, "wb") as f:
        f.write(data)


class BatchWriter:
    """PNG compression runs on a small thread pool (zlib releases the GIL): the arrays are materialised in the calling thread,
    the files are complete after finish().  With png_encoder="gpu" the score maps and the processed query / reference images are converted
    and compressed on the device (PngEncoder): write_out only queues that work, the pool threads wait for its event and write the bytes."""

    def __init__(self, cfg, phase: str, img_mean_std: torch.Tensor, device: torch.device, workers: int = 4, png_encoder: str = "host",
                 png_compression: str = "fast"):
        if phase not in ("test", "predict"):
            raise ValueError(f"Phase {phase} not supported. Has to be a Lightening phase test/predict.")
        if png_encoder not in PNG_ENCODERS:
            raise ValueError(f"png_encoder {png_encoder!r} not supported: host | gpu")
        self.png_encoder = png_encoder
        if png_compression not in PNG_COMPRESSIONS:
            raise ValueError(f"png_compression {png_compression!r} not supported: fast | compact")
        self.png_compression = png_compression
        self._png = PngEncoder(png_compression) if png_encoder == "gpu" else None
        self._stats = {"png_gpu_files": 0, "png_host_files": 0}
        self.cfg = cfg
        self.out_dir = Path(cfg.logger[phase].out_dir)
        self.write_config = cfg.logger[phase].write.config
        self.write_flag = cfg.logger[phase].write.flag
        m = cfg.model.predict.metric
        self.encoder = ScoreMapEncoder(m.type, m.min, m.max, self.write_config.score_map_colour_mode, device)
        self.img_mean_std = img_mean_std.detach().float().cpu()
        from concurrent.futures import ThreadPoolExecutor
        self._pool = ThreadPoolExecutor(max_workers=max(1, workers))
        self._pending = []
        # batch_writer.py:42-45: attention images only when the model returns the weights
        self.write_attn = bool(self.write_flag["attn_weights"]) and bool(cfg.model.need_attn_weights)
        self.out_dir_dict = {"batch": Path(self.out_dir, "batch")}
        self.phase = phase
        # score_map_gt (batch_writer.py:137-152): the test phase's GT maps, batch_input["query/score_map"] on the device
        kinds = ("item_path_json", "image_query", "image_reference", "attn_weights") + (("score_map_gt",) if phase == "test" else ())
        if self.write_flag["batch"]:
            for k in self.write_flag.keys():
                if k not in ("batch", "score_map_prediction") and self.write_flag[k] and k in kinds:
                    self.out_dir_dict[k] = Path(self.out_dir_dict["batch"], k)
                    self.out_dir_dict[k].mkdir(parents=True, exist_ok=True)

    # batch_writer.py:63-104
    def write_out(self, batch_input, batch_output, local_rank: int, batch_idx: int) -> List[str]:
        written: List[str] = []
        if self.write_flag["score_map_prediction"]:
            written += self._write_score_map_prediction(batch_input, batch_output, local_rank, batch_idx)
        if self.phase == "test" and self.write_flag.get("score_map_gt", False):
            written += self._write_score_map_gt(batch_input, local_rank, batch_idx)
        if self.write_flag["item_path_json"]:
            out_path = self.out_dir_dict["item_path_json"] / f"r{local_rank}_B{str(batch_idx).zfill(4)}.json"
            item_paths = dict(batch_input["item_paths"])
            if len(item_paths["reference/cross/imgs"]) > 0:  # transpose to (B, N_ref) like batch_writer.py:160-163
                item_paths["reference/cross/imgs"] = np.array(item_paths["reference/cross/imgs"]).T.tolist()
            with open(out_path, "w") as f:
                json.dump(item_paths, f, indent=2)
            written.append(str(out_path))
        if self.write_flag["image_query"]:
            stems = [name_stem(p) for p in batch_input["item_paths"]["query/img"]]
            paths = []
            for b, (stem, img) in enumerate(zip(stems, batch_input["query/img"])):
                path = self.out_dir_dict["image_query"] / f"r{local_rank}_B{batch_idx:04}_b{b:03}_{stem}.png"
                paths.append(path)
                if self._png is None:
                    self._save(path, self._de_norm_u8(img))
                written.append(str(path))
            if self._png is not None and paths:
                self._save_gpu(paths, denorm_to_rgb8(batch_input["query/img"][: len(paths)], self.img_mean_std))
        if self.write_flag["image_reference"] and len(batch_input["item_paths"]["reference/cross/imgs"]) > 0:
            stems = [name_stem(p) for p in batch_input["item_paths"]["query/img"]]
            ref_paths = np.array(batch_input["item_paths"]["reference/cross/imgs"]).T  # (B, N_ref)
            paths, picks = [], []
            for b, stem in enumerate(stems):
                d = self.out_dir_dict["image_reference"] / f"r{local_rank}_B{batch_idx:04}_b{b:03}_{stem}" / "cross"
                d.mkdir(parents=True, exist_ok=True)
                for ref_idx, (rp, img) in enumerate(zip(ref_paths[b], batch_input["reference/cross/imgs"][b])):
                    path = d / f"ref{ref_idx:02}_{name_stem(rp)}.png"
                    if self._png is None:
                        self._save(path, self._de_norm_u8(img))
                    else:
                        paths.append(path)
                        picks.append((b, ref_idx))
                    written.append(str(path))
            if self._png is not None and paths:
                refs = batch_input["reference/cross/imgs"]
                n_ref = int(refs.shape[1])
                flat = refs.reshape((-1,) + tuple(refs.shape[2:]))
                if picks != [(b, r) for b in range(int(refs.shape[0])) for r in range(n_ref)]:
                    flat = flat[torch.tensor([b * n_ref + r for b, r in picks], device=flat.device)]
                self._save_gpu(paths, denorm_to_rgb8(flat, self.img_mean_std))
        if self.write_attn and len(batch_input["item_paths"]["reference/cross/imgs"]) > 0:
            written += self._write_attn_weights(batch_input, batch_output, local_rank, batch_idx)
        return written

    def _write_attn_weights(self, batch_input, batch_output, local_rank, batch_idx) -> List[str]:
        """batch_writer.py:202-261 with check_patch_mode="centre": per query, the (N_ref, h, w) attention of its centre patch."""
        written = []
        table = colormap_table("turbo")
        stems = [name_stem(p) for p in batch_input["item_paths"]["query/img"]]
        ref_paths = np.array(batch_input["item_paths"]["reference/cross/imgs"]).T  # (B, N_ref)
        amap = batch_output["attn_weights_map_ref_cross"]                           # (B, h, w, N_ref, h, w)
        th, tw = amap.shape[1:3]
        for b, stem in enumerate(stems):
            d = self.out_dir_dict["attn_weights"] / f"r{local_rank}_B{batch_idx:04}_b{b:03}_{stem}" / "cross"
            d.mkdir(parents=True, exist_ok=True)
            maps = amap[b, th // 2, tw // 2].detach().float().cpu().numpy()        # (N_ref, h, w)
            for ref_idx, (rp, m) in enumerate(zip(ref_paths[b], maps)):
                path = d / f"ref{ref_idx:02}_{name_stem(rp)}.png"
                self._save(path, attn2rgb(m, table))
                written.append(str(path))
        return written

    def write_reference_use(self, batch_input, batch_output, local_rank: int, batch_idx: int) -> List[str]:
        """this_main.reference_use_images: per query, under batch/reference_use/<the attention images' directory name>/cross, ref<k>_<name>.png =
        the (h, w) map of the share of each query patch's attention that reference k took, and focus.png = focus_map of the entropy; both
        through the turbo table on [0, 1], at the size the attention images have."""
        share, entropy = batch_output["ref_use_share"], batch_output["ref_use_entropy"]  # (B, N_ref, h, w), (B, h, w) on the device
        B, n_ref, h, w = (int(v) for v in share.shape)
        if getattr(self, "_turbo", None) is None or self._turbo.device != share.device:
            self._turbo = torch.from_numpy(colormap_table("turbo").reshape(-1)).to(share.device)
        rgb = unit_to_rgb8(torch.cat([share.reshape(B * n_ref, h, w), focus_map(entropy, n_ref)], dim=0), self._turbo)
        stems = [name_stem(p) for p in batch_input["item_paths"]["query/img"]]
        ref_paths = np.array(batch_input["item_paths"]["reference/cross/imgs"]).T  # (B, N_ref)
        paths = []
        for b, stem in enumerate(stems):
            d = self.out_dir_dict["batch"] / "reference_use" / f"r{local_rank}_B{batch_idx:04}_b{b:03}_{stem}" / "cross"
            d.mkdir(parents=True, exist_ok=True)
            paths += [d / f"ref{k:02}_{name_stem(rp)}.png" for k, rp in enumerate(ref_paths[b])]
        paths += [self.out_dir_dict["batch"] / "reference_use" / f"r{local_rank}_B{batch_idx:04}_b{b:03}_{stem}" / "cross" / "focus.png"
                  for b, stem in enumerate(stems)]
        if self._png is not None:
            self._save_gpu(paths, rgb)
        else:
            host = rgb.cpu().numpy()
            for i, path in enumerate(paths):
                self._save(path, host[i])
        return [str(p) for p in paths]

    def _save(self, path, arr: np.ndarray) -> None:
        self._stats["png_host_files"] += 1
        self._pending.append(self._pool.submit(save_png, path, np.ascontiguousarray(arr)))

    def _save_gpu(self, paths, pixels: torch.Tensor) -> None:
        """Device integer images -> files at `paths`: the encode and its copy to pinned memory are queued here, waited for in the pool."""
        if len(paths) != int(pixels.shape[0]):
            raise ValueError("num of output paths and images are not equal")
        handle = self._png.encode_async(pixels)
        self._stats["png_gpu_files"] += len(paths)
        for i, path in enumerate(paths):
            self._pending.append(self._pool.submit(save_png_bytes, path, handle, i))

    def _save_score_maps(self, paths, score: torch.Tensor) -> None:
        if self._png is not None:
            self._save_gpu(paths, self.encoder.device_image(score))
            return
        imgs = self.encoder(score)
        for b, path in enumerate(paths):
            self._save(path, imgs[b])

    def stats(self) -> Dict[str, int]:
        """Files queued so far by encoder: {"png_gpu_files", "png_host_files"}."""
        return dict(self._stats)

    def finish(self) -> None:
        """Waits for every queued file (re-raises the first failure)."""
        pending, self._pending = self._pending, []
        for f in pending:
            f.result()

    def _de_norm_u8(self, img_chw: torch.Tensor) -> np.ndarray:
        """de_norm_img + u8 (utils/misc/image.py:25-34, utils/io/images.py:20-23): x*std + mean, *255, truncated to uint8."""
        x = img_chw.detach().float().cpu().permute(1, 2, 0)
        x = x * self.img_mean_std[3:][None, None] + self.img_mean_std[:3][None, None]
        return (x.numpy() * 255.0).astype(np.uint8)

    def _write_score_map_prediction(self, batch_input, batch_output, local_rank, batch_idx) -> List[str]:
        written = []
        stems = [name_stem(p) for p in batch_input["item_paths"]["query/img"]]
        for key in [k for k in batch_output.keys() if k.startswith("score_map")]:
            d = Path(self.out_dir_dict["batch"], key)
            d.mkdir(parents=True, exist_ok=True)
            if len(stems) != len(batch_output[key]):
                raise ValueError("num of query images and score maps are not equal")
            paths = [d / f"r{local_rank}_B{batch_idx:04}_b{b:03}_{stem}.png" for b, stem in enumerate(stems)]
            self._save_score_maps(paths, batch_output[key])
            written += [str(p) for p in paths]
        return written


    def _write_score_map_gt(self, batch_input, local_rank, batch_idx) -> List[str]:
        stems = [name_stem(p) for p in batch_input["item_paths"]["query/img"]]
        if len(stems) != len(batch_input["query/score_map"]):
            raise ValueError("num of query images and score maps are not equal")
        paths = [self.out_dir_dict["score_map_gt"] / f"r{local_rank}_B{batch_idx:04}_b{b:03}_{stem}.png" for b, stem in enumerate(stems)]
        self._save_score_maps(paths, batch_input["query/score_map"])
        return [str(p) for p in paths]


def group_summary_rows(rows):
    """score_summariser.py:197-250: the per-image rows ([scene_name, rendered_dir, image_name, ...], in scoring order) of each
    <dataset>/<method>.csv: (dataset, method, its rows sorted by the three key columns), datasets and methods in order of first appearance.
    The score summary and the score-pool CSVs (pooling.py) both come through here, so they hold the same images in the same order."""
    part = ScoreSummariser._part
    methods, datasets = [], []
    for r in rows:
        parts = r[1].split("/")
        m, d = part(parts, -6), part(parts, -5)
        if m not in methods:
            methods.append(m)
        if d not in datasets:
            datasets.append(d)
    for d in datasets:
        for m in methods:
            group = [r for r in rows if (m in r[1] or m == "unknown") and (d in r[1] or d == "unknown")]
            group.sort(key=lambda r: (r[0], r[1], r[2]))
            yield d, m, group


class ScoreSummariser:
    """SummaryWriterPredictedOnlineTestPrediction: per-image mean scores -> score_summary/<dataset_type>/<rendering_method>.csv."""

    def __init__(self, metric_type: str, metric_min: float, dir_out):
        if metric_type == "ssim":
            metric_str = f"{metric_type}_-1_1" if metric_min == -1 else f"{metric_type}_0_1"
        else:
            metric_str = f"{metric_type}"
        self.columns = ["scene_name", "rendered_dir", "image_name", f"pred_{metric_str}"]
        self.csv_dir = Path(dir_out).expanduser() / "score_summary"
        self.csv_dir.mkdir(parents=True, exist_ok=True)
        self.rows: List[list] = []

    @staticmethod
    def _part(parts: Sequence[str], idx: int) -> str:
        return parts[idx] if -len(parts) <= idx < len(parts) else "unknown"  # the reference raises IndexError on such short paths

    def update(self, batch_input, batch_output, means: torch.Tensor = None) -> None:
        """score_summariser.py:166-195.  `means` = per-image means already reduced on the device (cs_forward's mean output); when
        absent they are taken from the single score-map entry like the reference does."""
        paths = batch_input["item_paths"]["query/img"]
        keys = [k for k in batch_output.keys() if k.startswith("score_map")]
        if len(keys) != 1:
            raise ValueError(f"Expect exactly one ref_type: self/cross, but got {keys}.")
        scores = means if means is not None else batch_output[keys[0]].mean(dim=[-1, -2])
        scores = scores.detach().float().cpu().tolist()
        for p, s in zip(paths, scores):
            parts = p.split("/")
            rendered = os.path.join(*parts[:-2]) if len(parts) > 2 else ""
            self.rows.append([self._part(parts, -5), rendered, parts[-1].replace("frame_", ""), s])

    def summarise(self) -> List[str]:
        """score_summariser.py:197-250: group by rendered_dir components, sort, write with float_format "%.4f"."""
        written = []
        for d, m, rows in group_summary_rows(self.rows):
            out_dir = self.csv_dir / d
            out_dir.mkdir(parents=True, exist_ok=True)
            path = out_dir / f"{m}.csv"
            with open(path, "w", newline="") as f:
                w = csv.writer(f, lineterminator="\n")
                w.writerow(self.columns)
                for r in rows:
                    w.writerow([r[0], r[1], r[2], "%.4f" % r[3]])
            written.append(str(path))
        return written

    def __len__(self) -> int:
        return len(self.rows)
