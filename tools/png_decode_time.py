"""cs_op_png_decode alone: HIP events round the call for a window of PNG files, beside PIL on the same files.

Three sets: 540x720 RGB photos (smooth + sigma 8 noise) written by PIL, the same images written by the device encoder (cs_op_png_encode: fixed
Huffman / stored blocks, one IDAT chunk per 16 KiB), and 518x518 gray16 maps.  Per set one JSON line: ms per call, microseconds per image and
literals + match bytes per second for the whole window and for I = 8 (what the window buys), PIL's ms per image on one thread and images/s on an
8-thread pool, and the host's own cost per file (read + probe + pinned copy) through decode.ImageDecoder.
usage: python tools/png_decode_time.py [--window 64] [--maps 8] [--reps 5]"""
import argparse, ctypes as C, io, json, os, sys, tempfile, time
from concurrent.futures import ThreadPoolExecutor
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, REPO)
from PIL import Image
from crossscore_amd import _lib
from crossscore_amd.decode import ImageDecoder, probe_png, read_image_u8, read_metric_map_u16

ap = argparse.ArgumentParser()
ap.add_argument("--window", type=int, default=64)
ap.add_argument("--maps", type=int, default=8)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
lib = _lib.load()
rng = np.random.Generator(np.random.PCG64(1)); yy, xx = np.mgrid[0:540, 0:720]
def img(i):
    a = np.stack([127 + 100 * np.sin(xx / (17.0 + i) + i), 127 + 100 * np.cos(yy / (23.0 + i)), (xx + yy + 31 * i) % 256], axis=2)
    return (a + rng.normal(0, 8, a.shape)).clip(0, 255).astype(np.uint8)
def pil_bytes(a):
    b = io.BytesIO(); Image.fromarray(a).save(b, format="PNG"); return b.getvalue()
def device_encoded(arrs, kind):
    px = torch.from_numpy(np.stack(arrs).view(np.int16) if kind == _lib.PNG_GRAY16 else np.stack(arrs)).cuda()
    I, H, W = px.shape[:3]
    slot = lib.cs_png_bound(kind, H, W)
    out = torch.zeros((I, slot), dtype=torch.uint8, device="cuda"); ln = torch.zeros((I,), dtype=torch.int32, device="cuda")
    work = torch.empty((lib.cs_png_workspace_bytes(kind, I, H, W),), dtype=torch.uint8, device="cuda")
    _lib.check(lib.cs_op_png_encode(C.c_void_p(px.data_ptr()), kind, I, H, W, H * W * (2 if kind == _lib.PNG_GRAY16 else 3), C.c_void_p(out.data_ptr()), slot,
                                    C.c_void_p(ln.data_ptr()), C.c_void_p(work.data_ptr()), None))
    torch.cuda.synchronize()
    o, l = out.cpu().numpy(), ln.cpu().numpy()
    return [o[i, :l[i]].tobytes() for i in range(I)]

def time_call(files, kind, h, w, reps):
    """median ms of cs_op_png_decode on these files (HIP events), after checking every status word and the pixels of file 0"""
    tabs = [probe_png(f) for f in files]
    n = len(files)
    lengths = np.array([len(f) for f in files], dtype=np.uint32); offsets = np.zeros(n, dtype=np.uint64); offsets[1:] = np.cumsum(lengths.astype(np.uint64))[:-1]
    so = np.zeros(n + 1, dtype=np.uint32); so[1:] = np.cumsum([len(t[1]) for t in tabs]); total = int(lengths.sum())
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    d = [dev(np.frombuffer(b"".join(files), np.uint8)), dev(offsets), dev(lengths), dev(np.concatenate([t[1] for t in tabs])), dev(so)]
    es = 2 if kind == _lib.PNG_GRAY16 else 3
    pix = torch.empty((n, h * w * es), dtype=torch.uint8, device="cuda"); st = torch.empty((n,), dtype=torch.int32, device="cuda")
    work = torch.empty((lib.cs_png_decode_workspace_bytes(kind, n, h, w, total),), dtype=torch.uint8, device="cuda")
    ms = []
    for _ in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(lib.cs_op_png_decode(*(C.c_void_p(t.data_ptr()) for t in d), total, n, kind, h, w, C.c_void_p(pix.data_ptr()), h * w * es,
                                        C.c_void_p(st.data_ptr()), C.c_void_p(work.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        e1.record(); e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    assert not st.cpu().numpy().any(), st.cpu().numpy()
    want = (read_metric_map_u16 if kind == _lib.PNG_GRAY16 else read_image_u8)(io.BytesIO(files[0]))
    got = pix[0].cpu().numpy()
    assert np.array_equal(got.view(np.uint16).reshape(h, w) if kind == _lib.PNG_GRAY16 else got.reshape(h, w, 3), want)
    return float(np.median(ms[1:]))

photos = [img(i) for i in range(args.window)]
maps = [(np.clip(0.5 + 0.4 * np.sin(xx[:518, :518] / 40.0 + i) * np.cos(yy[:518, :518] / 30.0), 0, 1) * 65534 + rng.integers(0, 200, (518, 518))).astype(np.uint16)
        for i in range(args.maps)]
sets = [("pil_rgb_540x720", [pil_bytes(a) for a in photos], _lib.PNG_RGB8, 540, 720),
        ("device_encoder_rgb_540x720", device_encoded(photos, _lib.PNG_RGB8), _lib.PNG_RGB8, 540, 720),
        ("pil_gray16_518x518", [pil_bytes(m) for m in maps], _lib.PNG_GRAY16, 518, 518)]
tmp = tempfile.mkdtemp(prefix="pngdec_")
for name, files, kind, h, w in sets:
    out_bytes = h * (1 + w * (2 if kind == _lib.PNG_GRAY16 else 3))  # literals + match bytes per image
    reader = read_metric_map_u16 if kind == _lib.PNG_GRAY16 else read_image_u8
    t = time.perf_counter()
    for f in files[:8]: reader(io.BytesIO(f))
    pil_ms = (time.perf_counter() - t) / 8 * 1e3
    with ThreadPoolExecutor(8) as pool:
        t = time.perf_counter(); list(pool.map(lambda f: reader(io.BytesIO(f)), files)); pil_pool = len(files) / (time.perf_counter() - t)
    paths = []
    for i, f in enumerate(files):
        paths.append(os.path.join(tmp, f"{name}_{i}.png")); open(paths[-1], "wb").write(f)
    with ThreadPoolExecutor(8) as pool:
        dec = ImageDecoder("cuda", pool)
        dec.decode(paths, kind == _lib.PNG_GRAY16).check()
        torch.cuda.synchronize(); t = time.perf_counter(); hd = dec.decode(paths, kind == _lib.PNG_GRAY16); host_ms = (time.perf_counter() - t) * 1e3; hd.check()
    line = {"set": name, "files": len(files), "mean_file_bytes": int(np.mean([len(f) for f in files])), "pil_ms_per_image_one_thread": round(pil_ms, 2),
            "pil_images_per_sec_8_threads": round(pil_pool, 1), "decoder_host_ms_per_file_read_probe_pinned_copy_launch": round(host_ms / len(files), 3)}
    for n in sorted({len(files), min(8, len(files))}, reverse=True):
        ms = time_call(files[:n], kind, h, w, args.reps)
        line[f"I{n}"] = {"ms_per_call": round(ms, 3), "us_per_image": round(1e3 * ms / n, 1), "images_per_sec": round(1e3 * n / ms, 1),
                         "stream_bytes_per_sec": round(n * out_bytes / (ms * 1e-3))}
    print(json.dumps(line), flush=True)
