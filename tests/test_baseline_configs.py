"""Every BASELINE.json configuration at its full size on the GPU: cfg-1 through the predict driver, cfg-3 at B=8,
cfg-4 at 16 items per GPU and at B=2 against the oracle, cfg-5 at B=2.  Where the fp32 oracle would take minutes the checks are
the size-independent properties of the path: batch items never interact (task/core.py:134-161 keeps B outermost, attention is
per sample), so (a) an item's score map is bit-identical whatever batch it sits in, (b) permuting the items permutes the outputs,
and item 0 of the seeded batch is the committed golden of the reference itself (tests/golden/g2, g3: same seed, same item)."""
import json
import os
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from crossscore_amd import synth  # noqa: E402
from crossscore_amd.config import load_config, model_config  # noqa: E402
from crossscore_amd.model import CrossScoreNet  # noqa: E402
from oracle import crossscore_oracle as orc  # noqa: E402
from nets import MAE_TARGET, MAE_TOL, MAX_TOL, check_compact, make_net  # noqa: E402

VITS, VITB = "facebook/dinov2-small", "facebook/dinov2-base"


def _run(net, q, r):
    out = net(torch.from_numpy(q).cuda(), torch.from_numpy(r).cuda(), False, 0, False)["score_map_ref_cross"]
    torch.cuda.synchronize()
    return out


def _properties(net, q, r, score):
    """finite, in the sigmoid range, deterministic, permutation-equivariant over the batch (bitwise)."""
    assert torch.isfinite(score).all() and float(score.min()) >= 0.0 and float(score.max()) <= 1.0
    B = q.shape[0]
    perm = np.roll(np.arange(B), 1)
    again = _run(net, q[perm].copy(), r[perm].copy())
    assert torch.equal(again, score[torch.from_numpy(perm).cuda()])


@pytest.mark.parametrize("seed", [1, 7])
def test_cfg2_bf16_operands_at_batch8(seed):
    """BASELINE configs[1] as BASELINE words it -- ViT-S/14, 518x518, 5 refs, bs=8, **bf16** operands (cs_config.operand_dtype = 1; the path's
    default is fp16) -- on two seeds: every item of the batch is bit-identical to the same item scored alone (batch invariance in this operand
    mode too), and items 0, 3 and 7 are held to north_star's MAE < 1e-3 against the fp32 oracle on the host.  The measured MAEs are printed:
    DESIGN.md 2 states the margin to the bound (r5 measured 7.6e-4 on seed 1, item 0)."""
    net, arch, sd = make_net(VITS, seed)
    net.operand_dtype = "bf16"
    q, r = synth.make_inputs_shard(0, 8, 5, 518, 518, seed)
    score = _run(net, q, r)
    assert score.shape == (8, 518, 518) and net.nonfinite_count() == 0
    for i in range(8):
        assert torch.equal(_run(net, q[i:i + 1].copy(), r[i:i + 1].copy())[0], score[i]), i
    torch.set_num_threads(min(os.cpu_count() or 1, 32))
    W = orc.to_torch(sd)
    maes = {}
    for i in (0, 3, 7):
        ref = orc.forward(W, dict(enc_heads=arch.enc_heads), torch.from_numpy(q[i:i + 1]), torch.from_numpy(r[i:i + 1]))["score_map_ref_cross"][0]
        d = (score[i].cpu() - ref).abs()
        maes[i] = (float(d.mean()), float(d.max()))
    print(f"cfg-2 bf16 operands, seed {seed}: " + ", ".join(f"item {i}: MAE {m:.2e} max {x:.2e}" for i, (m, x) in maes.items()))
    assert all(m < MAE_TOL for m, _ in maes.values()), maes


def test_cfg3_vitb_10refs_batch8(golden_dir):
    """BASELINE configs[2]: ViT-B/14, 518x518, 10 refs, bs=8 (I = 88 images, cross-attention Lk = 13 690, decoder dh = 96)."""
    g = np.load(os.path.join(golden_dir, "g2_vitb_518_n10.npz"))
    seed = int(g["seed"])
    net, arch, sd = make_net(VITB, seed)
    q, r = synth.make_inputs_shard(0, 8, 10, 518, 518, seed)
    score = _run(net, q, r)
    assert score.shape == (8, 518, 518)
    mae_rows, mae_grid, dmean = check_compact(g, score[:1])  # item 0 = the reference's own golden
    assert mae_rows < MAE_TARGET and mae_grid < MAE_TARGET and dmean < 1e-4, (mae_rows, mae_grid, dmean)
    one = _run(net, q[:1], r[:1])
    assert torch.equal(one[0], score[0])  # the same item alone: bitwise
    _properties(net, q, r, score)


def test_cfg3_shape_vitb_bf16_operands_vs_reference_golden(golden_dir):
    """BASELINE words cfg-2 "bf16"; the same operand mode on the ViT-B path (256 x 256 tile GEMMs with fp32-residual / GELU epilogues, dh = 64
    encoder and dh = 96 decoder attention over 13 690 keys, all with bf16 MFMA forms): item 0 of cfg-3 (B = 1) against the reference's own
    golden g2, inside north_star's 1e-3."""
    g = np.load(os.path.join(golden_dir, "g2_vitb_518_n10.npz"))
    seed = int(g["seed"])
    net, arch, sd = make_net(VITB, seed)
    net.operand_dtype = "bf16"
    q, r = synth.make_inputs_shard(0, 1, 10, 518, 518, seed)
    score = _run(net, q, r)
    assert net.nonfinite_count() == 0
    mae_rows, mae_grid, dmean = check_compact(g, score)
    print(f"cfg-3 shape, bf16 operands vs g2: MAE rows {mae_rows:.2e} grid {mae_grid:.2e} mean diff {dmean:.2e}")
    assert mae_rows < MAE_TOL and mae_grid < MAE_TOL and dmean < 1e-3, (mae_rows, mae_grid, dmean)


def test_cfg4_vitb_5refs_vs_oracle_and_16_per_gpu():
    """BASELINE configs[3]: ViT-B/14, 518x518, 5 refs, global bs=128 = 16 items per GPU.  B=2 against the fp32 oracle on the host,
    then one rank's 16 items: the first two must be bit-identical to the B=2 forward (shard-equivalence: concatenated shard outputs
    == single-GPU output), and the batch is permutation-equivariant."""
    seed = 4
    net, arch, sd = make_net(VITB, seed)
    q, r = synth.make_inputs_shard(0, 16, 5, 518, 518, seed)
    s2 = _run(net, q[:2], r[:2])
    torch.set_num_threads(min(os.cpu_count() or 1, 32))
    ref = orc.forward(orc.to_torch(sd), dict(enc_heads=arch.enc_heads), torch.from_numpy(q[:2]), torch.from_numpy(r[:2]))["score_map_ref_cross"]
    d = (s2.cpu() - ref).abs()
    print(f"cfg4 B=2 vs oracle: MAE {float(d.mean()):.2e} max {float(d.max()):.2e}")
    assert float(d.mean()) < MAE_TOL and float(d.max()) < MAX_TOL
    s16 = _run(net, q, r)
    assert s16.shape == (16, 518, 518)
    assert torch.equal(s16[:2], s2)
    # a rank's shard inside the global batch: items [8, 16) scored alone == the same items of the 16-item forward
    s8 = _run(net, q[8:], r[8:])
    assert torch.equal(s8, s16[8:])
    _properties(net, q, r, s16)


def test_cfg5_1036_batch2(golden_dir):
    """BASELINE configs[4]: 1036x1036 query, 5 refs, bs=2 (T = 5477 encoder tokens per image, cross-attention 5476 x 27 380)."""
    g = np.load(os.path.join(golden_dir, "g3_vits_1036_n5.npz"))
    seed = int(g["seed"])
    net, arch, sd = make_net(VITS, seed)
    q, r = synth.make_inputs_shard(0, 2, 5, 1036, 1036, seed)
    score = _run(net, q, r)
    assert score.shape == (2, 1036, 1036)
    mae_rows, mae_grid, dmean = check_compact(g, score[:1])
    assert mae_rows < MAE_TARGET and mae_grid < MAE_TARGET and dmean < 1e-4, (mae_rows, mae_grid, dmean)
    assert torch.equal(_run(net, q[1:], r[1:])[0], score[1])
    _properties(net, q, r, score)


def test_cfg1_predict_plumbing_518(tmp_path):
    """BASELINE configs[0]: task/predict.py on a checkpoint, 1 query + 5 refs, short side 518 -- as a plumbing run of THIS build's
    predict driver (540x720 PNGs -> 518x690 like MFR_subset_demo frames; image directory -> GPU input stage -> forward -> PNG / CSV)
    checked against the oracle pipeline (oracle transforms + fp32 oracle forward on the host).  Seeded synthetic ViT-S weights in a
    Lightning-layout checkpoint: the released checkpoint is a git-LFS pointer and MFR_subset_demo is not in the image."""
    from PIL import Image

    from crossscore_amd.predict import predict
    from oracle import preprocess_oracle as po

    base = tmp_path / "data" / "gaussian" / "mfr" / "res_540" / "s00000" / "test" / "ours_1000"
    qd, rd = base / "renders", base / "gt"
    qd.mkdir(parents=True)
    rd.mkdir(parents=True)
    rng = np.random.Generator(np.random.PCG64(1))
    yy, xx = np.mgrid[0:540, 0:720]

    def img(i):
        a = np.stack([127 + 100 * np.sin(xx / (17.0 + i) + i), 127 + 100 * np.cos(yy / (23.0 + i)), (xx + yy + 31 * i) % 256], axis=2)
        return (a + rng.normal(0, 8, a.shape)).clip(0, 255).astype(np.uint8)

    Image.fromarray(img(0)).save(qd / "frame_00000.png")
    for i in range(5):
        Image.fromarray(img(i + 1)).save(rd / f"frame_{i:05}.png")
    arch = CrossScoreNet(model_config()).arch
    sd = synth.make_state_dict(arch, 1)
    ckpt = tmp_path / "run" / "ckpt" / "synthetic.ckpt"
    ckpt.parent.mkdir(parents=True)
    torch.save({"state_dict": {"model." + k: torch.from_numpy(v) for k, v in sd.items()}}, ckpt)
    cfg = load_config("default_predict", [f"data.dataset.query_dir={qd}", f"data.dataset.reference_dir={rd}", f"trainer.ckpt_path_to_load={ckpt}",
                                          "data.neighbour_config.deterministic=True", "logger.predict.write.config.score_map_colour_mode=gray"])
    t0 = time.perf_counter()
    res = predict(cfg, now="RUN")
    t_run = time.perf_counter() - t0
    png = [f for f in res["files"] if "/score_map_ref_cross/" in f][0]
    got = np.array(Image.open(png)).astype(np.float64) / 32767 - 1
    assert got.shape == (518, 686)  # 690 // 14 * 14: trailing pixels dropped (HF modeling_dinov2.py:141-149)
    q = po.preprocess_u8(np.array(Image.open(qd / "frame_00000.png")), (518, 690))[None]
    r = np.stack([po.preprocess_u8(np.array(Image.open(rd / f"frame_{i:05}.png")), (518, 690)) for i in range(5)])[None]
    torch.set_num_threads(min(os.cpu_count() or 1, 32))
    # (the predict driver's default position-embedding resize is the reference environment's scale_factor form: default_predict.yaml)
    ref = orc.forward(orc.to_torch(sd), dict(enc_heads=arch.enc_heads, pos_interp_legacy=True), torch.from_numpy(q), torch.from_numpy(r), False, 0)["score_map_ref_cross"][0].numpy()
    mae = float(np.abs(got - ref).mean())
    print(json.dumps({"cfg1_score_map_mae_vs_oracle_pipeline": mae, "driver_wall_s": round(t_run, 2), "csv_row": res["rows"][0]}))
    assert mae < MAE_TOL
    assert abs(float(res["rows"][0][-1]) - float(ref.mean())) < 1e-3  # the per-image mean the CSV row carries


def test_dinov2_giant_vs_oracle_and_batch_invariance():
    """facebook/dinov2-giant (C = 1536, 40 layers, 24 heads, SwiGLU MLP with 4096 hidden features; decoder heads of 192 channels) -- the backbone
    task/core.py:39-40 would load for model.backbone.from_pretrained=facebook/dinov2-giant.  The real depth at 224 x 224 (256 patches; the fp32
    oracle on the host takes the two images through 40 layers), B=1, N=1 against the oracle, then B=3, N=2: item-wise bitwise invariance."""
    net, arch, sd = make_net("facebook/dinov2-giant", 11)
    assert arch.swiglu and arch.ffn_hidden == 4096 and arch.hidden // arch.dec_heads == 192
    q, r = synth.make_inputs_shard(0, 1, 1, 224, 224, 11)
    score = _run(net, q, r)
    assert net.nonfinite_count() == 0
    ref = orc.forward(orc.to_torch(sd), dict(enc_heads=arch.enc_heads), torch.from_numpy(q), torch.from_numpy(r))["score_map_ref_cross"]
    d = (score.cpu() - ref).abs()
    print(f"dinov2-giant 224x224 vs oracle: MAE {float(d.mean()):.2e} max {float(d.max()):.2e}")
    assert float(d.mean()) < MAE_TOL and float(d.max()) < 2 * MAX_TOL, (float(d.mean()), float(d.max()))
    q3, r3 = synth.make_inputs_shard(0, 3, 2, 224, 224, 12)
    s3 = _run(net, q3, r3)
    one = _run(net, q3[1:2].copy(), r3[1:2].copy())
    assert torch.equal(one[0], s3[1])
    _properties(net, q3, r3, s3)


def test_dinov2_large_518_vs_oracle_and_batch_invariance():
    """Beyond BASELINE's two backbones: facebook/dinov2-large (C = 1024, 24 layers, 16 heads; decoder heads of 128 channels) at 518x518.
    B=1, N=1 against the fp32 oracle on the host (two images through 24 layers: ~20 s), then B=3, N=2: item-wise bitwise invariance."""
    net, arch, sd = make_net("facebook/dinov2-large", 9)
    q, r = synth.make_inputs_shard(0, 1, 1, 518, 518, 9)
    score = _run(net, q, r)
    assert net.nonfinite_count() == 0
    W = orc.to_torch(sd)
    ref = orc.forward(W, dict(enc_heads=arch.enc_heads), torch.from_numpy(q), torch.from_numpy(r))["score_map_ref_cross"]
    d = (score.cpu() - ref).abs()
    assert float(d.mean()) < MAE_TOL and float(d.max()) < 2 * MAX_TOL, (float(d.mean()), float(d.max()))
    q3, r3 = synth.make_inputs_shard(0, 3, 2, 518, 518, 10)
    s3 = _run(net, q3, r3)
    one = _run(net, q3[1:2].copy(), r3[1:2].copy())
    assert torch.equal(one[0], s3[1])
    _properties(net, q3, r3, s3)


def test_bench_plain_run_dumps_the_last_step(tmp_path, golden_dir):
    """`bench.py` without --full: the headline keys and no extra leg; --dump-outputs writes the score maps of the last timed step, whose item 0
    is the committed golden of the reference itself (tests/golden/g1: bench's seed, same item)."""
    import subprocess
    import sys

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "dump"
    res = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    r = json.loads(lines[0])
    assert r["unit"] == "query-images/sec" and r["higher_is_better"] is True and r["dtype"] == "fp16" and r["steps"] == 3
    assert r["value"] > 0 and abs(r["value"] - 8 * 1e3 / r["ms_per_step"]) < 1e-6 * r["value"]
    assert not {"roofline", "cpu_baseline", "eager_baseline", "scaling_cfg4", "dtype_legs", "value_repeats"} & set(r)
    assert sorted(os.listdir(out)) == ["score_map_ref_cross.npy"]
    s = np.load(out / "score_map_ref_cross.npy")
    assert s.dtype == np.float32 and s.shape == (8, 518, 518) and np.isfinite(s).all()
    g = np.load(os.path.join(golden_dir, "g1_vits_518_n5.npz"))
    mae_rows, mae_grid, dmean = check_compact(g, torch.from_numpy(s[:1]))
    assert mae_rows < MAE_TARGET and mae_grid < MAE_TARGET and dmean < 1e-4, (mae_rows, mae_grid, dmean)
