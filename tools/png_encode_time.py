"""Device PNG encoder on one cfg-2 batch's default outputs (ViT-S, 518 x 518, 5 references, batch 8): 8 turbo score maps + 8 processed
query images + 40 processed reference images, all RGB.  Prints
  * the HIP-event time of cs_op_png_encode alone for the three groups (and for the 8 gray16 maps of score_map_colour_mode=gray), beside the
    event time of the same batch's forward and of the conversions that feed the encoder;
  * the produced file sizes against PIL's default output (Image.fromarray(a).save) for the same arrays.
The images are the generator of tools/predict_e2e.py (540 x 720, smooth structure + noise of sigma 8) through the real input stage.
Every group is encoded in the fast (cs_op_png_encode_ex flags 0) and the compact (flags 3) form; --parent-lib <libcrossscore_hip.so of the
parent commit> adds that library's cs_op_png_encode on the same arrays, the three forms alternating in three rounds."""
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
parent = None
if "--parent-lib" in sys.argv:
    parent = C.CDLL(sys.argv[sys.argv.index("--parent-lib") + 1])
    for name in ("cs_png_bound", "cs_png_workspace_bytes", "cs_op_png_encode"):
        getattr(parent, name).restype, getattr(parent, name).argtypes = _lib.SYMBOLS[name]
def raw_encode(pixels, flags=0, use=None):
    kind, bpp = (_lib.PNG_GRAY16, 2) if pixels.dtype == torch.int16 else (_lib.PNG_RGB8, 3)
    I, H, W = (int(v) for v in pixels.shape[:3])
    slot = lib.cs_png_bound(kind, H, W)
    o = torch.empty((I, slot), dtype=torch.uint8, device=dev); ln = torch.empty((I,), dtype=torch.int32, device=dev)
    ws = torch.empty((lib.cs_png_workspace_bytes(kind, I, H, W),), dtype=torch.uint8, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    def go():
        args = (C.c_void_p(pixels.data_ptr()), kind, I, H, W, H * W * bpp, C.c_void_p(o.data_ptr()), slot, C.c_void_p(ln.data_ptr()), C.c_void_p(ws.data_ptr()), st)
        rc = use.cs_op_png_encode(*args) if use is not None else lib.cs_op_png_encode_ex(*args, flags)
        assert rc == 0, rc
        return ln
    return go

res = {"forward_ms": round(t_fwd, 3), "convert_ms": round(t_conv, 3), "score_std": round(float(score.std()), 4)}
FORMS = [("fast", 0, None), ("compact", 3, None)] + ([("parent", 0, parent)] if parent is not None else [])
total = {f: [0.0, 0.0, 0.0] for f, _, _ in FORMS}
for name, px in groups.items():
    arr = px.cpu().numpy(); arr = arr.view(np.uint16) if arr.dtype == np.int16 else arr
    pil, t0 = [], time.perf_counter()
    for a in arr:
        buf = io.BytesIO(); Image.fromarray(a).save(buf, format="PNG"); pil.append(buf.tell())
    t_pil = (time.perf_counter() - t0) / len(arr)
    raw = int(np.prod(arr.shape[1:])) * arr.dtype.itemsize
    row = {"group": name, "images": len(arr), "bytes_pil_mean": int(np.mean(pil)), "pil_host_ms_per_image": round(1e3 * t_pil, 1)}
    times = {f: [] for f, _, _ in FORMS}
    for rnd in range(3):  # the forms alternate: a drift of the box shows as spread inside every form, not as a difference between them
        for form, flags, use in FORMS:
            t, ln = timed(raw_encode(px, flags, use))
            times[form].append(round(t, 3))
            if name != "score_map_gray16": total[form][rnd] += t
            if rnd == 0:
                ours = ln.cpu().numpy().astype(np.int64)
                row.update({f"bytes_{form}_mean": int(ours.mean()), f"{form}_ratio_to_pil": round(float(ours.sum() / np.sum(pil)), 3),
                            f"{form}_ratio_to_raw": round(float(ours.mean() / raw), 3)})
    row.update({f"encode_ms_{form}": times[form] for form in times})
    print(json.dumps(row), flush=True)
# the asynchronous form end to end (encode + copy of the slots to pinned memory), as the writer queues it
for form in ("fast", "compact"):
    pe = PngEncoder(form)
    t_async, _ = timed(lambda: [pe.encode_async(groups[k]) for k in ("score_map_rgb", "image_query", "image_reference")], k=5)
    res[f"encode_plus_copy_ms_default_outputs_{form}"] = round(t_async, 3)
res.update({f"encode_ms_default_outputs_{form}": [round(v, 3) for v in total[form]] for form in total})
res["compact_encode_over_forward"] = round(min(total["compact"]) / t_fwd, 2)
print(json.dumps(res), flush=True)
