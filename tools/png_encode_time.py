"""Device PNG encoder on one cfg-2 batch's default outputs (ViT-S, 518 x 518, 5 references, batch 8): 8 turbo score maps + 8 processed
query images + 40 processed reference images, all RGB.  Prints
  * the HIP-event time of cs_op_png_encode alone for the three groups (and for the 8 gray16 maps of score_map_colour_mode=gray), beside the
    event time of the same batch's forward and of the conversions that feed the encoder;
  * the produced file sizes against PIL's default output (Image.fromarray(a).save) for the same arrays.
The images are the generator of tools/predict_e2e.py (540 x 720, smooth structure + noise of sigma 8) through the real input stage."""
import ctypes as C, io, json, os, sys, time
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, REPO)
from PIL import Image
from crossscore_amd import _lib, synth
from crossscore_amd.config import model_config
from crossscore_amd.data import IMAGENET_MEAN_STD, InputStage
from crossscore_amd.model import CrossScoreNet
from crossscore_amd.writers import PngEncoder, ScoreMapEncoder, denorm_to_rgb8

dev = torch.device("cuda", 0)
rng = np.random.Generator(np.random.PCG64(1)); yy, xx = np.mgrid[0:540, 0:720]
def img(i):
    a = np.stack([127 + 100 * np.sin(xx / (17.0 + i) + i), 127 + 100 * np.cos(yy / (23.0 + i)), (xx + yy + 31 * i) % 256], axis=2)
    return (a + rng.normal(0, 8, a.shape)).clip(0, 255).astype(np.uint8)
stage = InputStage(dev, resize_short_side=518, crop_size=518)
def processed(n, off):
    out = torch.empty((n, 3, 518, 518), dtype=torch.float32, device=dev)
    for i in range(n): stage(img(off + i), out[i])
    return out
tq, tr = processed(8, 0), processed(40, 100).reshape(8, 5, 3, 518, 518)
net = CrossScoreNet(model_config()); net.load_numpy_state_dict(synth.make_state_dict(net.arch, 1)); net = net.cuda()

def timed(fn, k=10, warm=2):
    for _ in range(warm): r = fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(k): r = fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / k, r

with torch.no_grad():
    t_fwd, out = timed(lambda: net(tq, tr, False, 0, False))
score = out["score_map_ref_cross"].contiguous()
ms = torch.tensor(list(IMAGENET_MEAN_STD), dtype=torch.float32)
enc_rgb, enc_gray = ScoreMapEncoder("ssim", 0, 1, "rgb", dev), ScoreMapEncoder("ssim", 0, 1, "gray", dev)
t_conv, groups = timed(lambda: {"score_map_rgb": enc_rgb.device_image(score), "image_query": denorm_to_rgb8(tq, ms),
                                "image_reference": denorm_to_rgb8(tr.reshape(40, 3, 518, 518), ms)})
groups["score_map_gray16"] = enc_gray.device_image(score)

lib = _lib.load()
def raw_encode(pixels):
    kind, bpp = (_lib.PNG_GRAY16, 2) if pixels.dtype == torch.int16 else (_lib.PNG_RGB8, 3)
    I, H, W = (int(v) for v in pixels.shape[:3])
    slot = lib.cs_png_bound(kind, H, W)
    o = torch.empty((I, slot), dtype=torch.uint8, device=dev); ln = torch.empty((I,), dtype=torch.int32, device=dev)
    ws = torch.empty((lib.cs_png_workspace_bytes(kind, I, H, W),), dtype=torch.uint8, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    def go():
        _lib.check(lib.cs_op_png_encode(C.c_void_p(pixels.data_ptr()), kind, I, H, W, H * W * bpp, C.c_void_p(o.data_ptr()), slot, C.c_void_p(ln.data_ptr()),
                                        C.c_void_p(ws.data_ptr()), st))
        return ln
    return go

res = {"forward_ms": round(t_fwd, 3), "convert_ms": round(t_conv, 3), "score_std": round(float(score.std()), 4)}
total = 0.0
for name, px in groups.items():
    t, ln = timed(raw_encode(px))
    ours = ln.cpu().numpy().astype(np.int64)
    arr = px.cpu().numpy(); arr = arr.view(np.uint16) if arr.dtype == np.int16 else arr
    pil, t0 = [], time.perf_counter()
    for a in arr:
        buf = io.BytesIO(); Image.fromarray(a).save(buf, format="PNG"); pil.append(buf.tell())
    t_pil = (time.perf_counter() - t0) / len(arr)
    raw = int(np.prod(arr.shape[1:])) * arr.dtype.itemsize
    if name != "score_map_gray16": total += t
    print(json.dumps({"group": name, "images": len(arr), "encode_ms": round(t, 3), "encode_us_per_image": round(1e3 * t / len(arr), 1),
                      "bytes_ours_mean": int(ours.mean()), "bytes_pil_mean": int(np.mean(pil)), "ratio_to_pil": round(float(ours.sum() / np.sum(pil)), 3),
                      "ratio_to_raw": round(float(ours.mean() / raw), 3), "pil_host_ms_per_image": round(1e3 * t_pil, 1)}), flush=True)
# the asynchronous form end to end (encode + copy of the slots to pinned memory), as the writer queues it
pe = PngEncoder()
t_async, _ = timed(lambda: [pe.encode_async(groups[k]) for k in ("score_map_rgb", "image_query", "image_reference")], k=5)
res.update({"encode_ms_default_outputs": round(total, 3), "encode_plus_copy_ms_default_outputs": round(t_async, 3),
            "encode_over_forward": round(total / t_fwd, 2)})
print(json.dumps(res), flush=True)
