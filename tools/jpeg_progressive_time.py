"""cs_op_jpeg_decode_ex with CS_JPEG_PROGRESSIVE alone: HIP events round the call for a window of progressive JPEG files, with the level
schedule on and forced off (cs_debug_jpeg_scan_levels), beside their baseline twins through the same call and PIL on the same bytes.

The images are tools/jpeg_decode_time.py's: 540x720 photo-like (smooth + sigma 8 noise), PIL, quality 90, 4:2:0, written progressive: without
restart markers, and with restart_marker_blocks=45 -- one MCU row per interval in the interleaved DC scans, 45 blocks per interval in the others
(PIL's restart_marker_rows writes a DRI before every scan of a progressive file, which cs_jpeg_probe_ex leaves to PIL).  Per set one JSON line:
per I (the window, and 8) the median ms per call of 5 after a warm-up for progressive with levels, progressive without, and the baseline twins,
measured alternately in one loop; PIL's ms per image on one thread and images/s on 8 threads over the progressive bytes; the host probe's
microseconds per file (it walks the whole file now).  Every status word is 0 and file 0's pixels are PIL's before anything is timed.
usage: python tools/jpeg_progressive_time.py [--window 64] [--reps 5]"""
import argparse, ctypes as C, io, json, os, sys, time
from concurrent.futures import ThreadPoolExecutor
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, REPO)
from PIL import Image
from crossscore_amd import _lib
from crossscore_amd.decode import probe_jpeg, read_image_u8

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

class Call:
    """one cs_op_jpeg_decode_ex call on these files, ready to be queued again and again"""
    def __init__(self, files, h, w):
        n = len(files)
        assert all(probe_jpeg(f, True)[0] is not None for f in files)
        lengths = np.array([len(f) for f in files], dtype=np.uint32); offsets = np.zeros(n, dtype=np.uint64); offsets[1:] = np.cumsum(lengths.astype(np.uint64))[:-1]
        self.total, self.n, self.h, self.w, self.files = int(lengths.sum()), n, h, w, files
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
        self.d = [dev(np.frombuffer(b"".join(files), np.uint8)), dev(offsets), dev(lengths)]
        self.pix = torch.empty((n, h * w * 3), dtype=torch.uint8, device="cuda"); self.st = torch.empty((n,), dtype=torch.int32, device="cuda")
        self.work = torch.empty((lib.cs_jpeg_decode_workspace_bytes_ex(n, h, w, self.total, _lib.JPEG_PROGRESSIVE),), dtype=torch.uint8, device="cuda")
    def run(self, levels):
        lib.cs_debug_jpeg_scan_levels(levels)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(lib.cs_op_jpeg_decode_ex(*(C.c_void_p(t.data_ptr()) for t in self.d), self.total, self.n, self.h, self.w, C.c_void_p(self.pix.data_ptr()),
                                            self.h * self.w * 3, C.c_void_p(self.st.data_ptr()), C.c_void_p(self.work.data_ptr()), _lib.JPEG_PROGRESSIVE,
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        e1.record(); e1.synchronize()
        lib.cs_debug_jpeg_scan_levels(1)
        return e0.elapsed_time(e1)
    def verify(self, levels):
        self.pix.fill_(0xA5); self.run(levels)
        assert not self.st.cpu().numpy().any(), self.st.cpu().numpy()
        assert np.array_equal(self.pix[0].cpu().numpy().reshape(self.h, self.w, 3), read_image_u8(io.BytesIO(self.files[0])))

photos = [img(i) for i in range(args.window)]
h, w = 540, 720
for name, kw in (("pil_q90_420_540x720_progressive", {}), ("pil_q90_420_540x720_progressive_restart_blocks_45", dict(restart_marker_blocks=45))):
    files = [pil_bytes(a, progressive=True, **kw) for a in photos]
    twins = [pil_bytes(a, **kw) for a in photos]
    t = time.perf_counter()
    for f in files[:8]: read_image_u8(io.BytesIO(f))
    pil_ms = (time.perf_counter() - t) / 8 * 1e3
    with ThreadPoolExecutor(8) as pool:
        t = time.perf_counter(); list(pool.map(lambda f: read_image_u8(io.BytesIO(f)), files)); pil_pool = len(files) / (time.perf_counter() - t)
    t = time.perf_counter()
    for f in files: probe_jpeg(f, True)
    probe_us = (time.perf_counter() - t) / len(files) * 1e6
    t = time.perf_counter()
    for f in twins: probe_jpeg(f, True)
    probe_twin_us = (time.perf_counter() - t) / len(twins) * 1e6
    line = {"set": name, "files": len(files), "mean_file_bytes": int(np.mean([len(f) for f in files])), "mean_twin_bytes": int(np.mean([len(f) for f in twins])),
            "pil_ms_per_image_one_thread": round(pil_ms, 2), "pil_images_per_sec_8_threads": round(pil_pool, 1),
            "probe_us_per_progressive_file": round(probe_us, 1), "probe_us_per_baseline_file": round(probe_twin_us, 1)}
    for n in sorted({len(files), min(8, len(files))}, reverse=True):
        prog, base = Call(files[:n], h, w), Call(twins[:n], h, w)
        prog.verify(1); prog.verify(0); base.verify(1)
        ms = {"levels": [], "serial": [], "baseline": []}
        for rep in range(args.reps + 1):  # alternating; the first round is the warm-up
            for key, call, lv in (("levels", prog, 1), ("serial", prog, 0), ("baseline", base, 1)):
                v = call.run(lv)
                if rep: ms[key].append(v)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        line[f"I{n}"] = {"progressive_levels_ms": round(med["levels"], 3), "progressive_one_scan_per_level_ms": round(med["serial"], 3),
                         "baseline_twins_same_call_ms": round(med["baseline"], 3), "progressive_levels_images_per_sec": round(1e3 * n / med["levels"], 1),
                         "baseline_images_per_sec": round(1e3 * n / med["baseline"], 1)}
    print(json.dumps(line), flush=True)
