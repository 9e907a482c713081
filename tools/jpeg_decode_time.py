"""cs_op_jpeg_decode alone: HIP events round the call for a window of baseline JPEG files, beside PIL on the same files.

Two sets of 540x720 photo-like images (smooth + sigma 8 noise) written by PIL at quality 90, 4:2:0: without restart markers (one wave decodes a
file) and with one MCU row per restart interval (the four waves of a file's workgroup share its intervals).  Per set one JSON line: ms per call,
microseconds per image and compressed bytes per second for the whole window and for I = 8 (what the window buys), PIL's ms per image on one
thread and images/s on an 8-thread pool, and the host's own cost per file (read + probe + pinned copy + launch) through decode.ImageDecoder.
usage: python tools/jpeg_decode_time.py [--window 64] [--reps 5]"""
import argparse, ctypes as C, io, json, os, sys, tempfile, time
from concurrent.futures import ThreadPoolExecutor
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, REPO)
from PIL import Image
from crossscore_amd import _lib
from crossscore_amd.decode import ImageDecoder, probe_jpeg, read_image_u8

ap = argparse.ArgumentParser()
ap.add_argument("--window", type=int, default=64)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
lib = _lib.load()
rng = np.random.Generator(np.random.PCG64(1)); yy, xx = np.mgrid[0:540, 0:720]
def img(i):
    a = np.stack([127 + 100 * np.sin(xx / (17.0 + i) + i), 127 + 100 * np.cos(yy / (23.0 + i)), (xx + yy + 31 * i) % 256], axis=2)
    return (a + rng.normal(0, 8, a.shape)).clip(0, 255).astype(np.uint8)
def pil_bytes(a, **kw):
    b = io.BytesIO(); Image.fromarray(a).save(b, format="JPEG", quality=90, subsampling=2, **kw); return b.getvalue()

def time_call(files, h, w, reps):
    """median ms of cs_op_jpeg_decode on these files (HIP events), after checking every status word and the pixels of file 0"""
    n = len(files)
    assert all(probe_jpeg(f)[0] is not None for f in files)
    lengths = np.array([len(f) for f in files], dtype=np.uint32); offsets = np.zeros(n, dtype=np.uint64); offsets[1:] = np.cumsum(lengths.astype(np.uint64))[:-1]
    total = int(lengths.sum())
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    d = [dev(np.frombuffer(b"".join(files), np.uint8)), dev(offsets), dev(lengths)]
    pix = torch.empty((n, h * w * 3), dtype=torch.uint8, device="cuda"); st = torch.empty((n,), dtype=torch.int32, device="cuda")
    work = torch.empty((lib.cs_jpeg_decode_workspace_bytes(n, h, w, total),), dtype=torch.uint8, device="cuda")
    ms = []
    for _ in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(lib.cs_op_jpeg_decode(*(C.c_void_p(t.data_ptr()) for t in d), total, n, h, w, C.c_void_p(pix.data_ptr()), h * w * 3, C.c_void_p(st.data_ptr()),
                                         C.c_void_p(work.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        e1.record(); e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    assert not st.cpu().numpy().any(), st.cpu().numpy()
    assert np.array_equal(pix[0].cpu().numpy().reshape(h, w, 3), read_image_u8(io.BytesIO(files[0])))
    return float(np.median(ms[1:]))

photos = [img(i) for i in range(args.window)]
sets = [("pil_q90_420_540x720", [pil_bytes(a) for a in photos]), ("pil_q90_420_540x720_restart_rows_1", [pil_bytes(a, restart_marker_rows=1) for a in photos])]
tmp = tempfile.mkdtemp(prefix="jpgdec_")
for name, files in sets:
    h, w = 540, 720
    t = time.perf_counter()
    for f in files[:8]: read_image_u8(io.BytesIO(f))
    pil_ms = (time.perf_counter() - t) / 8 * 1e3
    with ThreadPoolExecutor(8) as pool:
        t = time.perf_counter(); list(pool.map(lambda f: read_image_u8(io.BytesIO(f)), files)); pil_pool = len(files) / (time.perf_counter() - t)
    paths = []
    for i, f in enumerate(files):
        paths.append(os.path.join(tmp, f"{name}_{i}.jpg")); open(paths[-1], "wb").write(f)
    with ThreadPoolExecutor(8) as pool:
        dec = ImageDecoder("cuda", pool, jpeg=True)
        dec.decode(paths).check()
        torch.cuda.synchronize(); t = time.perf_counter(); hd = dec.decode(paths); host_ms = (time.perf_counter() - t) * 1e3; hd.check()
        assert not hd.host_paths and dec.jpeg_stats()["jpeg_decoded_gpu"] == 2 * len(files)
    mean_bytes = float(np.mean([len(f) for f in files]))
    line = {"set": name, "files": len(files), "mean_file_bytes": int(mean_bytes), "pil_ms_per_image_one_thread": round(pil_ms, 2),
            "pil_images_per_sec_8_threads": round(pil_pool, 1), "decoder_host_ms_per_file_read_probe_pinned_copy_launch": round(host_ms / len(files), 3)}
    for n in sorted({len(files), min(8, len(files))}, reverse=True):
        ms = time_call(files[:n], h, w, args.reps)
        line[f"I{n}"] = {"ms_per_call": round(ms, 3), "us_per_image": round(1e3 * ms / n, 1), "images_per_sec": round(1e3 * n / ms, 1),
                         "compressed_bytes_per_sec": round(n * mean_bytes / (ms * 1e-3))}
    print(json.dumps(line), flush=True)
