/* C ABI of libcrossscore_hip.so -- the MI355X (gfx950) CrossScore inference hot path.
 *
 * The reference (ActiveVisionLab/CrossScore) is pure Python and has no native interface; the boundary this
 * library sits behind is the model call
 *     CrossScoreNet.forward(query_img, ref_cross_imgs, need_attn_weights, need_attn_weights_head_id, norm_img)
 *         -> {"score_map_ref_cross", "attn_weights_map_ref_cross"}            (task/core.py:58-117)
 * made from CrossScoreLightningModule._core_step (task/core.py:265-272).  Each entry point below names the
 * reference code it replaces.  Plain pointers and sizes only: no torch / Python types cross this line.
 *
 * Ownership: the caller (PyTorch) owns every input / output / weight-source buffer; the library owns only its
 * packed fp16 weights and its workspace.  Threading: a handle is not thread-safe and serves one forward at a time (its
 * workspace is shared by consecutive calls); to keep several batches in flight create one handle per batch in flight (the
 * Python side does: crossscore_amd/pipeline.py) -- handles are independent, also across GPUs of one process (launcher state
 * is kept per device).  All work is enqueued on
 * the caller's hipStream_t (a forward that arrives on another stream than the previous one waits for it with an event: the
 * workspace is shared).  No entry point waits for the device or a stream except cs_finalize, cs_profile_*, cs_destroy,
 * cs_op_streams_overlap and the one-time creation of the encoder lanes' streams in a handle's first forward (which probes that
 * the lanes' streams overlap, ~1 ms):
 * the first forward of a new shape allocates (hipMalloc: position tables of a new patch grid, a larger workspace -- the old
 * one is retired behind an event and freed later), fills what it allocated on the caller's stream, and never overwrites or
 * frees memory that queued work may still read; calls of a shape seen before allocate nothing.  (Only a 17th distinct patch
 * grid, or a 65th distinct resize geometry in cs_preprocess_u8, drops the table cache behind a device synchronisation.)
 * Weights are fp32 at this boundary (cs_set_weight; cs_set_weight_typed also takes fp16 / bf16 sources and widens them): the
 * reference checkpoint stores fp32, and the library packs its own 16-bit copies in cs_finalize.  Every function returning int returns 0 on success; on failure
 * cs_last_error() describes it (CS_ERR_* below) and nothing was launched on the bad-argument paths.
 */
#ifndef CROSSSCORE_HIP_H
#define CROSSSCORE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cs_model* cs_handle;
typedef void* cs_stream; /* hipStream_t */

enum {
  CS_OK = 0,
  CS_ERR_BAD_ARG = 1,     /* shape / config the reference would also reject (ValueError / assert) */
  CS_ERR_UNSUPPORTED = 2, /* legal for the reference, not built here (e.g. head dim outside {16,48,64,96,128,192}) */
  CS_ERR_STATE = 3,       /* wrong call order (forward before finalize, missing weight) */
  CS_ERR_HIP = 4          /* HIP runtime error; message carries hipGetErrorString */
};

/* Architecture + the model.* config keys the forward consumes (config/model/model.yaml:1-32). */
typedef struct cs_config {
  int hidden;        /* C: Dinov2Config.hidden_size (384 small / 768 base), task/core.py:39 */
  int enc_layers;    /* Dinov2Config.num_hidden_layers */
  int enc_heads;     /* Dinov2Config.num_attention_heads (head dim hidden / enc_heads in {16,48,64,96,128}; DINOv2: 64) */
  int mlp_ratio;     /* 4 */
  int patch;         /* model.patch_size = 14 */
  int pos_grid;      /* sqrt(#position_embeddings - 1) = 37 */
  int pe_h, pe_w;    /* model.pos_enc.multi_view.{h,w} = 40,40 (bilinear, align_corners=True) */
  int dec_layers;    /* 2, model/cross_reference.py:38 */
  int dec_heads;     /* 8, model/cross_reference.py:31 */
  int do_self_attn;  /* model.decoder_do_self_attn */
  int do_short_cut;  /* model.decoder_do_short_cut */
  int act;           /* 0 sigmoid (metric.min == 0), 1 tanh (metric.min == -1), model/regression_layer.py:31-38 */
  float pow_p;       /* exponent after the activation; 1 = identity, model/regression_layer.py:40-62 */
  int enc_chunk_images; /* images per encoder pass (0 = library default) */
  int ln_fold;       /* encoder LayerNorms (HF modeling_dinov2.py:361-380) folded into the producing / consuming GEMM epilogues:
                      * 0 (default): by backbone width -- hidden 384: inside the token-panel kernel; hidden 768 / 1024: in the 256-tile GEMM's
                      *    epilogues for chunks of >= 256 rows (residual epilogues write 16-bit(x) + row partial sums, a row-statistics kernel,
                      *    QKV / fc1 apply rstd * (acc - mean * s) + c), separate LayerNorm kernels otherwise;
                      * 1: the 128-row kernel's folded epilogues everywhere (fp16 operands only; slower: A/B and tests);
                      * 2: separate LayerNorm kernels for the wide backbones */
  int lanes;         /* internal streams that run independent image chunks / batch groups concurrently: 0 = default (2), 1 = serial, up to 4 */
  int pos_interp_legacy; /* encoder position-embedding resize (grids other than 37 x 37, or H != W): 0 = F.interpolate(size=(h, w)), the installed
                       * transformers (>= 4.4x; what the goldens were generated with); 1 = scale_factor ((h + 0.1) / 37, (w + 0.1) / 37) as
                       * in the reference's pinned transformers 4.33.3 (environment.yaml:340): source coordinates shrink by h / (h + 0.1) */
  int enc_fused;      /* encoder layer structure: 0 = default: with hidden == 384 (ViT-S) each layer is QKV GEMM + attention + ONE
                       * token-panel kernel (out-projection, residual, norm2, fc1, GELU, fc2, residual and the next layer's norm1; the 4C
                       * hidden activations stay in registers), else the unfused kernels; 1 = always the unfused kernels */
  int operand_dtype;  /* 16-bit operand type of the MFMA kernels (activations between kernels, packed weights): 0 = IEEE half (default: 11 significant
                       * bits, finite to 65504; score-map MAE 1e-4 vs the fp32 reference), 1 = bfloat16 (8 bits, fp32's range; MAE 8e-4): the
                       * choice for a checkpoint whose activations leave the half range (trainer.precision = bf16-mixed in the predict driver).
                       * Accumulation, softmax statistics, LayerNorm, the residual stream and the outputs are fp32 either way. */
  int pe_interp_mode; /* model.pos_enc.multi_view.interpolate_mode, applied when the patch grid differs from (pe_h, pe_w) (model/positional_encoding.py:61-69,
                       * always with align_corners=True): 0 = bilinear (the reference default), 1 = bicubic.  torch rejects every other mode of a 4-D
                       * tensor with align_corners=True, so these two are all the reference can run. */
  int skip_finite_check; /* 0 = default: every forward ends with a pass over the score map that counts non-finite values into a device
                       * counter (cs_nonfinite_count; ~3 us); 1 = skip it */
  int swiglu;         /* encoder MLP: 0 = Dinov2MLP (fc1 -> GELU -> fc2, HF modeling_dinov2.py:286-297); 1 = Dinov2SwiGLUFFN (HF:300-316,
                       * Dinov2Config.use_swiglu_ffn: facebook/dinov2-giant): weights_in (2F x C) -> silu(x1) * x2 -> weights_out (C x F) with
                       * F = (int(hidden * mlp_ratio * 2 / 3) + 7) / 8 * 8, which must be a multiple of 64; the layer then runs as separate
                       * LayerNorm / GEMM launches with one elementwise launch for the gate (no token-panel kernel, no LayerNorm fold) */
} cs_config;

/* Replaces CrossScoreNet.__init__ (task/core.py:27-56). NULL on failure. */
cs_handle cs_create(const cs_config* cfg);
void cs_destroy(cs_handle h);
const char* cs_last_error(void);

/* Replaces load_state_dict for one tensor: `name` is the checkpoint key without the "model." prefix (ckpt layout:
 * SURVEY.md 8b), `data` fp32, row-major, host or device memory (is_device), `shape[ndim]` as in the state dict. */
int cs_set_weight(cs_handle h, const char* name, const float* data, int is_device, int ndim, const int64_t* shape);
/* The same for a source tensor of another storage type (SURVEY.md 8b's `dtype` argument): a half- or bfloat16-precision checkpoint is
 * widened to fp32 (exactly) on the way in. */
enum { CS_DTYPE_F32 = 0, CS_DTYPE_F16 = 1, CS_DTYPE_BF16 = 2 };
int cs_set_weight_typed(cs_handle h, const char* name, const void* data, int is_device, int dtype, int ndim, const int64_t* shape);
/* Number of tensors cs_finalize expects and the i-th expected name (for loaders / strict checking). */
int cs_num_weights(cs_handle h);
const char* cs_weight_name(cs_handle h, int i);
/* Packs weights to fp16 / fused layouts (QKV, both decoder layers' KV). Fails if a tensor is missing. */
int cs_finalize(cs_handle h);

/* Replaces CrossScoreNet.forward (task/core.py:58-117) with norm_img=False.
 *   query:  (B,3,H,W) fp32 device, contiguous;   refs: (B,N,3,H,W) fp32 device, contiguous
 *   score_out: (B, P*(H/P), P*(W/P)) fp32 device
 *   attn_out:  NULL, or (B, h, w, N, h, w) fp32 device = probabilities of head `head_id` of the LAST decoder
 *              layer's cross-attention (model/cross_reference.py:91-93)
 *   mean_out:  NULL, or (B) fp32 device = per-image mean of the score map (utils/io/score_summariser.py:180-192), formed inside the head's
 *              launch (no pass over the map); an item's mean has the same bits alone and at any position of any batch */
int cs_forward(cs_handle h, const float* query, const float* refs, int B, int N, int H, int W, float* score_out,
               float* attn_out, int head_id, float* mean_out, cs_stream stream);
/* Reference-feature cache.  In predict the N references of every query are drawn from one finite
 * reference_dir (dataloading/dataset/simple_reference.py:55-58, utils/neighbour/sampler.py:27-34), and a reference's
 * decoder input -- final LayerNorm of its DINOv2 tokens + multi-view PE, task/core.py:141-153,93-98 -- does not depend on the
 * query or on its view slot.  cs_encode_references encodes R images once into fp16 tokens (R, h*w, C); cs_forward_cached
 * scores B queries against gathered tokens (B, N, h*w, C).  Results are bit-identical to cs_forward on the same images; the
 * encoder work per query drops from 1+N images to 1 (a separate mode: it changes the algorithmic FLOPs). */
int cs_encode_references(cs_handle h, const float* imgs, int R, int H, int W, uint16_t* tokens_out, cs_stream stream);
int cs_forward_cached(cs_handle h, const float* query, const uint16_t* ref_tokens, int B, int N, int H, int W,
                      float* score_out, float* attn_out, int head_id, float* mean_out, cs_stream stream);
/* The same three forwards fed from DECODED uint8 images (SURVEY.md 8f-4 as worded: uint8 in, tokens out).  Replaces, together with the patch
 * embedding, the reference's CPU input transforms -- np.float32(img) / 255 (utils/io/images.py:14-29), T.Resize(short side, BILINEAR, antialias)
 * (task/predict.py:87-93, nvs_dataset.py:218-225), the deterministic / integer-patch crop (dataloading/transformation/crop.py:8-25,
 * nvs_dataset.py:227-241), T.Normalize (task/predict.py:68-74) -- inside the patch-embedding launch: no fp32 image tensor is written or read.  The
 * strip of pixels a patch row needs is formed in LDS by the operations of cs_op_preprocess_u8 in their order, so the token rows, and with them every
 * later value, are bit-identical to cs_op_preprocess_u8 + the fp32 entry point (tested).  query / refs / imgs are HOST arrays of descriptors (B; B * N,
 * item-major; R); an image's `data` is DEVICE memory and must stay valid until the stream has passed the call; data == NULL is the all-zero placeholder
 * image (nvs_dataset.py:459-470: zeros before T.Normalize).  Images of one call may differ in size and geometry, not in the H x W window.  mean3 /
 * std3 are HOST pointers.  CS_ERR_UNSUPPORTED when the handle does not run the one-launch patch embedding (patch 14, hidden a multiple of 384) or a
 * patch row reaches more source rows than the launch holds in LDS (1 170: a down-scale beyond ~70 x): cs_u8_input_supported asks beforehand. */
typedef struct cs_u8_image {
  const uint8_t* data;   /* device, HWC RGB, rows row_bytes apart; NULL: all-zero image */
  int h, w, row_bytes;   /* decoded size */
  int rs_h, rs_w;        /* size after T.Resize (== h, w: no resize) */
  int crop_y, crop_x;    /* top-left corner of the H x W window inside the resized image */
} cs_u8_image;
int cs_forward_u8(cs_handle h, const cs_u8_image* query, const cs_u8_image* refs, int B, int N, int H, int W, const float* mean3, const float* std3,
                  float* score_out, float* attn_out, int head_id, float* mean_out, cs_stream stream);
int cs_encode_references_u8(cs_handle h, const cs_u8_image* imgs, int R, int H, int W, const float* mean3, const float* std3, uint16_t* tokens_out,
                            cs_stream stream);
int cs_forward_cached_u8(cs_handle h, const cs_u8_image* query, const uint16_t* ref_tokens, int B, int N, int H, int W, const float* mean3,
                         const float* std3, float* score_out, float* attn_out, int head_id, float* mean_out, cs_stream stream);
/* 1 when the three calls above take this image geometry on this handle, 0 when not (then: cs_op_preprocess_u8 + the fp32 entry points) */
int cs_u8_input_supported(cs_handle h, const cs_u8_image* img, int H, int W);
/* Reference selection by DINOv2 similarity (this build's definition, the reference's sampler only draws at random).  An image's
 * descriptor is pooled from its decoder-input rows t (Np, C), 16 bit, exactly what cs_encode_references writes:
 *   mean   m[c] = (1 / Np) sum_p t[p][c]        fp32, in an order that depends on Np and C only (not on the launch's image count or the image's place)
 *   centre mu[c] = (1 / R) sum_r m_r[c]         over the R images of a bank (removes the pooled multi-view PE, a constant every image carries)
 *   unit   e = (m - mu) / max(|m - mu|, 1e-12)
 *   s(q, r) = sum_c e_q[c] e_r[c]               the same instruction sequence for every pair: equal bank rows give equal bits
 * and a query takes the N bank entries of largest s, in descending order, ties to the lower index, exclude[b] (when >= 0) left out.
 *   cs_op_token_descriptors   tokens (I, Np, C) 16 bit, dtype CS_DTYPE_F16 / CS_DTYPE_BF16 -> mean_out (I, C); C a multiple of 64, I <= 65535
 *   cs_op_descriptor_centre   mean (R, C) -> centre_out (C)
 *   cs_op_descriptor_unit     mean (I, C), centre (C) -> unit_out (I, C); a row equal to the centre gives zeros
 *   cs_op_select_references   q_unit (B, C), bank_unit (R, C) -> sim_out (B, R) (required here) and index_out (B, N) int32.  N <= 32 and
 *                             R <= 65536, else CS_ERR_UNSUPPORTED.  CS_ERR_BAD_ARG when N exceeds the eligible entries: R without `exclude`,
 *                             R - 1 with it (the array lives on the device and is not read by the host, so any query may carry an exclusion).
 *                             A query with fewer than N candidates (NaN similarities never qualify) gets -1 in the remaining places.
 *   cs_op_gather_tokens       out (B, N, Np, C) <- bank (R, Np, C) rows named by index (B, N), 16-byte vectors (Np * C a multiple of 8); an index
 *                             outside [0, R) reads nothing and its slot becomes zeros; B * N <= 65535
 * cs_forward_select* is cs_forward_cached* with the choice made on the device: behind the encoder the query's descriptors are pooled from the
 * 16-bit copy of its decoder input (the rounding cs_encode_references applies, so a query that is also a bank image gets that row's mean bit for
 * bit), the N entries are selected against bank_unit (R, C) / centre (C) and their rows of bank_tokens (R, Np, C) are gathered into the workspace;
 * decoder and head then run as in cs_forward_cached on those rows (bit-identical to it).  index_out (B, N) is required; sim_out NULL keeps the
 * similarities in the workspace.  Every pointer is device memory; nothing is copied to the host or waited for.  Debug taps: "select_query_mean",
 * "select_query_unit" fp32 (B, C). */
int cs_op_token_descriptors(const uint16_t* tokens, int I, int Np, int C, int dtype, float* mean_out, cs_stream stream);
int cs_op_descriptor_centre(const float* mean, int R, int C, float* centre_out, cs_stream stream);
int cs_op_descriptor_unit(const float* mean, int I, int C, const float* centre, float* unit_out, cs_stream stream);
int cs_op_select_references(const float* q_unit, int B, const float* bank_unit, int R, int C, const int32_t* exclude /* NULL or (B), -1 = none */,
                            int N, int32_t* index_out /* (B, N) */, float* sim_out /* (B, R) */, cs_stream stream);
int cs_op_gather_tokens(const uint16_t* bank, int R, int Np, int C, const int32_t* index, int B, int N, uint16_t* out, cs_stream stream);
int cs_forward_select(cs_handle h, const float* query, const uint16_t* bank_tokens, const float* bank_unit, const float* centre, int R,
                      const int32_t* exclude, int B, int N, int H, int W, float* score_out, float* attn_out, int head_id, float* mean_out,
                      int32_t* index_out, float* sim_out /* NULL or (B, R) */, cs_stream stream);
int cs_forward_select_u8(cs_handle h, const cs_u8_image* query, const uint16_t* bank_tokens, const float* bank_unit, const float* centre, int R,
                         const int32_t* exclude, int B, int N, int H, int W, const float* mean3, const float* std3, float* score_out,
                         float* attn_out, int head_id, float* mean_out, int32_t* index_out, float* sim_out, cs_stream stream);
/* Grouped banks (the test phase, where a query chooses among the images of its own scene).  A bank of R rows carries G groups:
 * group g is the rows offsets[g] .. offsets[g + 1] - 1, offsets[0] = 0, strictly increasing, offsets[G] <= R; the rows from offsets[G] on
 * belong to no group and are never selected.  Every group has its own centre -- the centre of an ungrouped bank made of that slice, bit for bit --
 * a bank row's unit uses its group's centre, query b the centre of its group query_group[b], and b is compared with the rows of that group only:
 * order, ties, the NaN rule and exclude[b] (a bank row; one outside the group has no effect) as above.  index_out holds bank rows, -1 where the
 * group ran out (N may exceed a group).  sim_out is (B, S), S the longest group: column j of query b is bank row offsets[query_group[b]] + j, the
 * columns behind its group a quiet NaN.  Every result equals, bit for bit, what the ungrouped calls give on the sliced group.
 * offsets (G + 1) and query_group (B) are HOST arrays: they are checked here, resolved per query and uploaded asynchronously on the call's stream
 * from a pinned slot; nothing is read back and no call waits.  CS_ERR_BAD_ARG for a group outside [0, G), offsets that do not start at 0 or do
 * not increase, offsets[G] > R, a blank_row inside a group or outside [-1, R); a refused call queues nothing.
 *   cs_op_group_descriptors          mean (R, C) -> centre_out (G, C) and unit_out (R, C), one launch each; unit_out's rows from offsets[G] on are
 *                                    left alone.  C a multiple of 64, R <= 65536
 *   cs_op_select_references_grouped  takes the queries' MEANS q_mean (B, C): the unit depends on the group.  N <= 32, R <= 65536
 *   cs_op_gather_tokens_ex           cs_op_gather_tokens with blank_row: an index outside [0, R) takes bank row blank_row's tokens when
 *                                    blank_row >= 0 (the encoder's tokens of the all-zero placeholder image), zeros when it is -1
 *   cs_forward_select_grouped*       cs_forward_select* on such a bank: centre is (G, C), sim_out NULL or (B, S); the gather takes blank_row.  With
 *                                    G = 1 over all rows and blank_row = -1 every output has the bits of cs_forward_select*: the ungrouped
 *                                    calls run the same kernels, told "one group of all R rows" by a NULL slice, and upload nothing. */
int cs_op_group_descriptors(const float* mean, int R, int C, const int32_t* offsets /* HOST (G + 1) */, int G, float* centre_out /* (G, C) */,
                            float* unit_out /* (R, C) */, cs_stream stream);
int cs_op_select_references_grouped(const float* q_mean, int B, const int32_t* query_group /* HOST (B) */, const float* bank_unit,
                                    const float* centre /* (G, C) */, const int32_t* offsets /* HOST (G + 1) */, int G, int R, int C,
                                    const int32_t* exclude /* NULL or (B), bank rows, -1 = none */, int N, int32_t* index_out /* (B, N) */,
                                    float* sim_out /* (B, S) */, cs_stream stream);
int cs_op_gather_tokens_ex(const uint16_t* bank, int R, int Np, int C, const int32_t* index, int B, int N, uint16_t* out, cs_stream stream,
                           int blank_row);
int cs_forward_select_grouped(cs_handle h, const float* query, const uint16_t* bank_tokens, const float* bank_unit, const float* centre, int R,
                              const int32_t* offsets, int G, const int32_t* query_group, int blank_row, const int32_t* exclude, int B, int N, int H,
                              int W, float* score_out, float* attn_out, int head_id, float* mean_out, int32_t* index_out, float* sim_out,
                              cs_stream stream);
int cs_forward_select_grouped_u8(cs_handle h, const cs_u8_image* query, const uint16_t* bank_tokens, const float* bank_unit, const float* centre,
                                 int R, const int32_t* offsets, int G, const int32_t* query_group, int blank_row, const int32_t* exclude, int B,
                                 int N, int H, int W, const float* mean3, const float* std3, float* score_out, float* attn_out, int head_id,
                                 float* mean_out, int32_t* index_out, float* sim_out, cs_stream stream);
/* Reference use of the next forward: the four outputs of cs_op_reference_use for the LAST decoder layer's cross-attention --
 * the one attn_out reports -- with Lq = Np = (H / patch)(W / patch): share, peak_prob, peak_index (B, N, h, w), entropy (B, h, w), device memory,
 * any of them NULL.  One-shot: the next cs_forward* call of any kind on this handle (plain, _u8, cached, select, grouped) takes the request, sizes it
 * by its own B, N, H, W, adds one launch ("ref_use" in cs_forward_stats) behind that cross-attention on the call's stream, and clears it whether
 * it succeeds or fails; cs_encode_references* leaves it armed.  All four NULL cancels.  Every other output of the forward keeps its bits. */
int cs_request_reference_use(cs_handle h, float* share, float* peak_prob, int32_t* peak_index, float* entropy);
/* Overflow report.  With fp16 operands an activation beyond 65504 becomes inf and reaches the score map as NaN (nothing clamps in
 * the hot kernels); every forward counts the non-finite values of its score map on the device.  This call waits for the handle's last
 * forward, returns the count since the previous call in *count and resets it: > 0 means "switch to operand_dtype = 1 (bf16)". */
int cs_nonfinite_count(cs_handle h, long long* count);
/* Bytes of library-owned workspace a forward of this shape needs (grown lazily, never shrunk). */
size_t cs_workspace_bytes(cs_handle h, int B, int N, int H, int W);

/* Lanes (internal streams that run independent image chunks of ONE forward side by side): cs_set_lanes limits the following forwards
 * to at most `lanes` (0 = as configured by cs_config.lanes; same launches, bit-identical results); cs_redraw_lane_streams gives the
 * handle's lane streams back so that the next forward draws and probes new ones (a set-up call: it waits for the lanes' work).  Together
 * they let the host check that a two-lane forward really beats the one-lane one and repair it if not (CrossScoreNet.calibrate_lanes):
 * two streams that passed the overlap probe can still end up serialised when other queues were created in between. */
int cs_set_lanes(cs_handle h, int lanes);
int cs_redraw_lane_streams(cs_handle h);
/* debug switch, process-wide (see cs_debug_* below): 1 = one stderr line per lane-stream candidate of the overlap probe (which streams a handle drew
 * and whether they dispatch side by side); default 0.  Replaces the CS_DEBUG_STREAMS environment read of rounds 3-5: the product path reads no
 * environment variable. */
void cs_debug_stream_probe_log(int on);

/* Launch census of the last cs_forward / cs_forward_cached / cs_encode_references on this handle: kernel launches, host wall time of the
 * call (all work is enqueued, nothing is waited for: this is what a rank's CPU thread pays per forward -- bench.py reports it per rank, the
 * reference pays the same kind of cost in Lightning's predict loop, task/predict.py:119-135) and, optionally, the launches by kernel as
 * "name=count ..." text (gemm256, gemm128, attn<dh>, panel, rowln, patch, im2col, ln*, cls, final_ln, ...; the parity tests use it to prove
 * which kernels a shape was routed to). */
int cs_forward_stats(cs_handle h, int* launches, double* host_ms, char* names, size_t names_bytes);

/* Stage-level taps for the parity tests (tests/test_hip_stages.py): with capture on, every forward of this handle also copies its
 * intermediate tensors into library-owned buffers (stream-ordered device-to-device copies; the first captured forward of a shape
 * allocates -- not for timed runs).  Names follow the reference's module outputs (tests/golden/make_golden.py hooks the same points):
 *   "embeddings"            fp32 (I, T, C)      Dinov2Embeddings output, HF modeling_dinov2.py:97-116; I = B * (1 + N) images in the
 *                                               reference's batch-major (query, refs...) order of task/core.py:134-138, T = 1 + h*w
 *   "enc_layer_<l>"         fp32 (I, T, C)      residual stream behind Dinov2Layer l, HF:361-380
 *   "featmap_query"         fp32 (B, h*w, C)    final LayerNorm of the query's patch tokens + multi-view PE, core.py:141-153,93-98
 *   "featmap_ref"           16 bit (B, N*h*w, C)  the same for the reference views (the decoder's memory), in the handle's operand type
 *   "dec<l>_out"            fp32 (B, h*w, C)    decoder layer l output, transformer.py:157-173
 *   "head_pre_activation"   fp32 (B, h*w, P*P)  head[2] output before the RegressionLayer, cross_reference.py:45-50
 * cs_debug_read copies a tap to dst (device memory of at least the tap's size; NULL = only report) on `stream` and reports its element
 * type (CS_DTYPE_*), rank and shape (4 entries).  CS_ERR_STATE when the last forwards captured no such tap. */
int cs_debug_capture(cs_handle h, int on);
int cs_debug_read(cs_handle h, const char* name, void* dst, size_t dst_bytes, int* dtype, int* ndim, int64_t* shape4, cs_stream stream);

/* Per-kernel-family timing with HIP events on the launch stream (for bench.py's roofline object).
 * Families = kernel symbols: 0..9 cs_gemm_kernel<epilogue> (either GEMM kernel), 16 + dh/16 cs_attn_kernel<dh>, 40 cs_panel_kernel,
 * 41 cs_patch_fused_kernel, 42 cs_rowln_kernel, 32 everything else (LayerNorm, im2col, CLS rows, tables).  `flops` = algorithmic FLOPs (2*M*N*K, 4*B*H*Lq*Lk*dh).  Two events per launch. */
int cs_profile_enable(cs_handle h, int on);
int cs_profile_read(cs_handle h, int family, double* total_ms, int* launches, double* flops);
/* algorithmic HBM bytes (operands and results once each) of the recorded launches of one family */
int cs_profile_read_bytes(cs_handle h, int family, double* bytes);

/* ---- single-op entry points (used by the parity tests; same kernels the forward launches) ------------- */
/* cs_debug_*: PROCESS-WIDE switches and taps for tests and measurement tools.  They are not part of the drop-in surface: a product caller never
 * needs them, and the "handles are independent" promise above holds only while nobody flips them under a running forward.
 * 16-bit operand type of the cs_op_* entry points below (a handle has its own cs_config.operand_dtype): 0 fp16 (default), 1 bf16 */
int cs_debug_set_op_operand_dtype(int dtype);
/* out = epilogue(bias + A[M,K] @ W[N,K]^T): see CsEpilogue in csrc/cs_common.h for `epi`. fp16 = raw uint16. */
int cs_op_gemm(const uint16_t* A, int lda, const uint16_t* W, int ldw, int M, int N, int K, const float* bias,
               const float* resid, int ldr, void* out, int ldc, int epi, const float* pos, int Np,
               int gw, int P, int act, float powp,
               /* LayerNorm fold (CsEpilogue 7-9): producer outputs, then consumer inputs; NULL / 0 when unused */
               uint16_t* out_f16, float* stats_out, int stats_sp, const float* ln_part, int ln_sp, const float* col_s,
               float ln_eps, cs_stream stream);
/* The head's last linear with its epilogue (model/regression_layer.py:26-62 activation, utils/misc/image.py:8-21 jigsaw) and, when the three
 * mean_* pointers are given, the per-image mean of the score map from the SAME launch (utils/io/score_summariser.py:180-192
 * score_map.mean(dim=[-1, -2])): score (M / Np, gh P, gw P) fp32; mean_part (M, 4 * ceil(P*P / 128)) fp32 scratch; mean_cnt (M / Np) uint32,
 * ZERO on entry and zero again on completion; mean_out (M / Np) fp32.  An image's mean has the same bits at any position of any batch. */
int cs_op_head_score(const uint16_t* A, int lda, const uint16_t* W, int ldw, int M, int K, const float* bias, float* score, int Np, int gw, int P,
                     int act, float powp, float* mean_part, unsigned* mean_cnt, float* mean_out, cs_stream stream);
/* softmax(QK^T/sqrt(dh))V for `batch` x `heads`; strides in elements; lse may be NULL. */
/* O = softmax(Q K^T / sqrt(dh)) V computed in the base-2 domain: p = 2^(q_scale * q.k - m).  The forward folds log2(e)/sqrt(dh) into its
 * Q projections and passes q_scale = 1 (Q arrives pre-multiplied); q_scale = 0 means log2(e)/sqrt(dh) applied here, to raw Q, at the
 * price of one more fp16 rounding of Q.  lse (optional, [batch][heads][Lq]) is in base-2 units of the scaled logits. */
int cs_op_attention(const uint16_t* Q, const uint16_t* K, const uint16_t* V, uint16_t* O, int ldq, int ldk, int ldv,
                    int ldo, long long q_bs, long long k_bs, long long v_bs, long long o_bs, int batch, int heads,
                    int Lq, int Lk, int dh, float q_scale, float* lse, cs_stream stream);
/* out[b][q][k] = 2^(q_scale * q.k - lse[b][head][q]) for ONE head, lse from cs_op_attention.  Q and K as there: row and batch strides
 * multiples of 8 elements, Lk * ldk below 2^30 (CS_ERR_BAD_ARG otherwise, before any launch). */
int cs_op_attention_weights(const uint16_t* Q, const uint16_t* K, int ldq, int ldk, long long q_bs, long long k_bs,
                            int batch, int heads, int Lq, int Lk, int dh, float q_scale, const float* lse, int head,
                            float* out, cs_stream stream);
/* Reference use: what a cross-attention over N references of Np keys each (key k = n Np + j) did with them, all heads, one
 * launch, no attention matrix in memory.  With s = q_scale * q.k (base 2, as cs_op_attention), e = s - lse[b][hd][q], p = 2^e and
 * pm[b][q][k] = (1 / heads) sum_hd p:
 *   share      (batch, N, Lq) fp32   sum_j pm[b][q][n Np + j]          peak_prob  (batch, N, Lq) fp32   max_j pm[b][q][n Np + j]
 *   peak_index (batch, N, Lq) int32  the j of that maximum, the lowest on equal values
 *   entropy    (batch, Lq) fp32      (1 / heads) sum_hd sum_k -p e, in bits
 * lse is cs_op_attention's, used as written.  Any output may be NULL (all NULL: nothing is launched).  Q and K as for cs_op_attention_weights
 * (CS_ERR_BAD_ARG before any launch otherwise), K rows hold the heads side by side (column hd * dh); a dh outside 16, 48, 64, 96, 128, 192 is
 * CS_ERR_UNSUPPORTED.  Operand type: cs_debug_set_op_operand_dtype. */
int cs_op_reference_use(const uint16_t* Q, const uint16_t* K, int ldq, int ldk, long long q_bs, long long k_bs, int batch, int heads, int Lq, int N,
                        int Np, int dh, float q_scale, const float* lse, float* share, float* peak_prob, int32_t* peak_index, float* entropy,
                        cs_stream stream);
int cs_op_layernorm(const float* x, int M, int C, const float* gamma, const float* beta, float eps, float* out_f32,
                    uint16_t* out_f16, cs_stream stream);
/* Row statistics of the LayerNorm folded into the 256-tile GEMM (cs_config.ln_fold = 0 on hidden 768 / 1024): part (M, sp, 2) partial (sum,
 * sum of squares) of every row's 64-column slices as the CS_EPI_RESID_F32_LN epilogue of that kernel writes them (sp = C / 64) ->
 * stat (rows_padded, 2) = (mean, 1 / sqrt(var + eps)), rows [M, rows_padded) zero (the consuming epilogue fetches whole 256-row tiles). */
int cs_op_ln_finalize(const float* part, int M, int rows_padded, int sp, int C, float eps, float* stat, cs_stream stream);
/* The gate of Dinov2SwiGLUFFN (HF modeling_dinov2.py:311-315; cs_config.swiglu) as the forward launches it: in place on M rows of 16-bit values
 * (the op operand type) `ld` elements apart, x[m][j] = silu(x[m][j]) * x[m][F + j] for j < F, fp32 arithmetic and one rounding; the second half
 * of each row and the elements behind 2 F are not written.  F and ld multiples of 8 (16-byte accesses), ld >= 2 F. */
int cs_op_silu_mul(uint16_t* x, int M, int F, int ld, cs_stream stream);
int cs_op_im2col(const float* x, uint16_t* out, int I, int H, int W, int P, int Kp, cs_stream stream);
/* The patch embedding exactly as the forward runs it (HF modeling_dinov2.py:141-149: conv patchify = im2col + GEMM, + position rows), with
 * (centred != 0) or without the mean-centred operand form: x (I,3,H,W), w (C,3,P,P), bias (C), pos (1 + Np, C) -> out (I * (1 + Np), C) fp32,
 * patch rows only.  Test entry point (allocates and synchronises). */
int cs_op_patch_embed(const float* x, const float* w, const float* bias, const float* pos, int I, int H, int W, int P, int C, int centred,
                      float* out, cs_stream stream);
/* The same patch embedding in ONE launch (csrc/patch.hip: image strip -> mean-centred 16-bit tile in LDS -> MFMA -> token rows; no im2col
 * matrix in memory), the form cs_forward uses for 14-pixel patches when C is a multiple of 384 and the LayerNorm-folded epilogues are off.
 * Arguments and result as cs_op_patch_embed(centred = 1); CS_ERR_BAD_ARG for other shapes.  Replaces HF modeling_dinov2.py:141-149. */
int cs_op_patch_embed_fused(const float* x, const float* w, const float* bias, const float* pos, int I, int H, int W, int P, int C,
                            float* out, cs_stream stream);
/* The same launch fed from I decoded uint8 images of one size and geometry (test entry point of the one-pass input stage, cs_forward_u8):
 * out = cs_op_patch_embed_fused applied to cs_op_preprocess_u8's output of every image, bit for bit. */
int cs_op_patch_embed_fused_u8(const uint8_t* imgs, int I, int in_h, int in_w, int row_bytes, int rs_h, int rs_w, int crop_y, int crop_x, int H, int W,
                               const float* mean3, const float* std3, const float* w, const float* bias, const float* pos, int P, int C, float* out,
                               cs_stream stream);
/* debug switch, process-wide (see cs_debug_* above): 0 = cs_forward goes back to im2col + GEMM for the patch embedding; default 1 */
void cs_debug_patch_fused_enable(int on);
/* Input stage: device uint8 HWC image (3 channels, rows in_row_bytes apart) -> fp32 CHW [3][out_h][out_w], the
 * tensor cs_forward consumes.  Same operations, in the same order, as the reference's CPU transforms: x/255 (utils/io/images.py:14-29),
 * antialiased bilinear resize to (rs_h, rs_w) (T.Resize, task/predict.py:87-93; skipped when equal to the input size), crop window
 * (crop_y, crop_x, out_h, out_w) of the resized image (dataloading/transformation/crop.py:8-25, nvs_dataset.py:227-241), then
 * (v - mean) / std (T.Normalize, task/predict.py:68-74).  mean3 / std3 are HOST pointers; scratch (device, in_h*rs_w*3 floats) is
 * needed only when resizing.  Filter tables of the last size pair are cached in the library (not thread-safe, like the handle). */
int cs_op_preprocess_u8(const uint8_t* img, int in_h, int in_w, int in_row_bytes, int rs_h, int rs_w, int crop_y, int crop_x, int out_h,
                        int out_w, const float* mean3, const float* std3, float* out, float* scratch, cs_stream stream);
/* Output stage: score map -> the integer images the reference's writers store (PNG compression stays on the host).
 * gray16: metric_map_write, utils/io/images.py:49-63 (signed_range 1: (m+1)*32767 for the SSIM intrinsic range, 0: m*65535), truncated.
 * rgb: gray2rgb, utils/misc/image.py:37-52 (Normalize(vmin,vmax), 256-entry colormap, u8 truncation); lut256x3 = the colormap's byte
 * table on the device (matplotlib "turbo" in the reference). */
int cs_op_score_to_gray16(const float* score, long long n, int signed_range, uint16_t* out, cs_stream stream);
int cs_op_score_to_rgb(const float* score, long long n, float vmin, float vmax, const uint8_t* lut256x3, uint8_t* out, cs_stream stream);
/* PNG files from the device.  I device images of one size and one kind -> I complete PNG files in device memory, file i at
 * out + i * slot_bytes, lengths[i] bytes long.  Replaces the compression half of the reference's writers: imageio.imwrite behind
 * metric_map_write (utils/io/images.py:49-63) and behind the image outputs of batch_writer.py:117-135; the integer images come from
 * cs_op_score_to_gray16 / cs_op_score_to_rgb / cs_op_denorm_to_rgb8.  kind CS_PNG_GRAY16: native-endian uint16, one sample per pixel (bit depth 16,
 * colour type 0); CS_PNG_RGB8: uint8 HWC (bit depth 8, colour type 2).  Rows are contiguous, images image_stride_bytes apart.
 * Every byte of a file is produced on the device (signature, IHDR, IDAT framing, zlib header, deflate data, Adler-32, chunk CRCs, IEND) in two
 * launches, whatever I is; the call does not wait for the device.  Guaranteed: a valid PNG whose decoded pixels equal the input exactly, and
 * bytes that depend on the image's pixels, size and kind alone (not on I, its position in the batch or the other images).  NOT guaranteed:
 * byte equality with any other encoder (PIL, imageio, libpng) -- the stream is cut into independent 16-KiB segments (one IDAT chunk each,
 * fixed-Huffman or stored blocks, Sub filter), so files are larger than zlib's.
 * 1 <= H, W <= 4096 (CS_ERR_UNSUPPORTED above), 1 <= I <= 65535.  slot_bytes >= the bound of the size; workspace: device, 16-byte aligned, at
 * least the workspace size of (kind, I, H, W).  The two size functions are host arithmetic (no device is touched; 0 for sizes the encoder does
 * not take); bad arguments are rejected before anything is launched. */
enum { CS_PNG_GRAY16 = 0, CS_PNG_RGB8 = 1 };
size_t cs_png_bound(int kind, int H, int W);
size_t cs_png_workspace_bytes(int kind, int I, int H, int W);
int cs_op_png_encode(const void* pixels, int kind, int I, int H, int W, long long image_stride_bytes, uint8_t* out, size_t slot_bytes,
                     uint32_t* lengths, void* workspace, cs_stream stream);
/* cs_op_png_encode with opt-in compression flags; flags == 0 is cs_op_png_encode byte for byte, flags outside 0 .. 3 are CS_ERR_BAD_ARG
 * (decided on the host before anything is launched).  The contract above holds for every flags value, with flags joining pixels, size and
 * kind in what an image's bytes depend on.
 * CS_PNG_ADAPTIVE_FILTER: each row takes the filter type 0 .. 4 whose filtered bytes f have the smallest sum of min(f, 256 - f) over the row
 * (integers; ties to the lowest type; the row above row 0 and the bytes left of the first pixel are zero; Paeth ties in the order a, b, c).
 * CS_PNG_DYNAMIC: each 16-KiB segment is priced exactly in four forms -- stored, fixed Huffman with the segment's LZ77 tokens (the flags == 0
 * form), dynamic Huffman with those tokens, dynamic Huffman with literals only -- and the smallest is written; a later form of that list wins
 * only when it is strictly smaller in bytes.  No segment is therefore longer than its stored form and no file longer than its flags == 0
 * file with the same filter, so cs_png_bound and cs_png_workspace_bytes hold for every flags value as they are. */
enum { CS_PNG_DYNAMIC = 1, CS_PNG_ADAPTIVE_FILTER = 2 };
int cs_op_png_encode_ex(const void* pixels, int kind, int I, int H, int W, long long image_stride_bytes, uint8_t* out, size_t slot_bytes,
                        uint32_t* lengths, void* workspace, cs_stream stream, int flags);
/* PNG files decoded on the device (csrc/pngdec.hip): the mirror of cs_op_png_encode.  I compressed files of one
 * decoded size (H, W) and one output kind -> I images in device memory, image i at pixels + i * image_stride_bytes with contiguous rows:
 * CS_PNG_RGB8 uint8 HWC from colour type 2 / depth 8, colour type 6 / depth 8 (alpha dropped) and colour type 0 / depth 8 (the sample
 * replicated); CS_PNG_GRAY16 native-endian uint16 from colour type 0 / depth 16.  Non-interlaced files only; any number of IDAT chunks, split
 * at any byte; stored, fixed and dynamic deflate blocks; all five filter types.  Everything else is not built: cs_png_probe says so
 * (CS_ERR_UNSUPPORTED) and the caller decodes that file elsewhere.
 * cs_png_probe is host arithmetic over the file's bytes (no device is touched): signature, chunk framing within n, IHDR; it fills info and,
 * when spans is not NULL, the (offset, length) of every IDAT payload relative to the file's first byte.  CS_ERR_BAD_ARG for framing that runs
 * past the end (or more IDAT chunks than max_spans; info->num_idat then holds the count).
 * cs_op_png_decode: files is ONE device buffer of total_file_bytes bytes holding the files back to back, file i at file_offsets[i],
 * file_lengths[i] long, its spans at spans[span_offsets[i] .. span_offsets[i + 1]) (all four arrays in device memory).  One launch, one
 * workgroup per file; the call does not wait for the device.  status[i] (device) is 0 for a complete, verified image -- CRC-32 of IHDR and of
 * every IDAT chunk, Adler-32 of the zlib stream, stream length exactly H * (1 + row bytes) -- or one of CS_PNGDEC_*; a file with a non-zero
 * status has written no pixel and has not disturbed the other files of the call.  The kernel re-checks every span against its file's length and
 * never reads past a file, so untrusted bytes cannot make it fault.  workspace: device, 16-byte aligned, cs_png_decode_workspace_bytes(...)
 * bytes (host arithmetic; 0 for kinds and sizes the decoder does not take).  1 <= H, W <= 4096 (CS_ERR_UNSUPPORTED above), 1 <= I <= 65535. */
typedef struct cs_png_info {
  int width, height, color_type, bit_depth, interlace;
  int kind;      /* CS_PNG_GRAY16 / CS_PNG_RGB8, -1 when the decoder does not take the file */
  int num_idat;  /* IDAT chunks in the file */
  unsigned long long idat_bytes;
} cs_png_info;
typedef struct cs_png_span { uint32_t offset, length; } cs_png_span;
enum {
  CS_PNGDEC_OK = 0,
  CS_PNGDEC_BAD_CRC = 1,         /* IHDR's or an IDAT chunk's CRC-32 */
  CS_PNGDEC_BAD_ADLER = 2,       /* Adler-32 of the inflated stream */
  CS_PNGDEC_BAD_ZLIB_HEADER = 3, /* CMF / FLG: method, window, check bits, preset dictionary */
  CS_PNGDEC_BAD_BLOCK_TYPE = 4,  /* reserved block type 3 */
  CS_PNGDEC_BAD_STORED_LEN = 5,  /* LEN / NLEN of a stored block disagree */
  CS_PNGDEC_BAD_CODE = 6,        /* over-subscribed or incomplete code, too many lengths, bad repeat, no end-of-block code */
  CS_PNGDEC_BAD_SYMBOL = 7,      /* bits that are no code of the set, length symbols 286 / 287, distance symbols 30 / 31 */
  CS_PNGDEC_BAD_DISTANCE = 8,    /* a distance before the start of the stream */
  CS_PNGDEC_STREAM_SHORT = 9,    /* the stream ends before H * (1 + row bytes) */
  CS_PNGDEC_STREAM_LONG = 10,    /* ... or goes on behind it */
  CS_PNGDEC_BAD_FILTER = 11,     /* filter type above 4 */
  CS_PNGDEC_INPUT_EXHAUSTED = 12,/* the IDAT bytes end inside the stream */
  CS_PNGDEC_HEADER_MISMATCH = 13,/* IHDR's size or format is not the call's (H, W, kind) */
  CS_PNGDEC_BAD_FRAMING = 14     /* signature, IHDR framing or a span outside its file */
};
int cs_png_probe(const uint8_t* file, size_t n, cs_png_info* info, cs_png_span* spans, int max_spans);
size_t cs_png_decode_workspace_bytes(int kind, int I, int H, int W, size_t total_file_bytes);
int cs_op_png_decode(const uint8_t* files, const uint64_t* file_offsets, const uint32_t* file_lengths, const cs_png_span* spans,
                     const uint32_t* span_offsets, size_t total_file_bytes, int I, int kind, int H, int W, void* pixels, long long image_stride_bytes,
                     uint32_t* status, void* workspace, cs_stream stream);
/* Baseline JPEG files decoded on the device (csrc/jpegdec.hip).  I compressed files of one decoded size (H, W)
 * -> I uint8 HWC RGB images in device memory (gray replicated: what data.read_image_u8 makes of PIL's array), image i at
 * pixels + i * image_stride_bytes with contiguous rows.  The contract: the pixels PIL (libjpeg-turbo: jpeg_idct_islow, fancy upsampling) gives,
 * exactly, or a status word and no pixel.  Accepted: SOF0, 8-bit samples, one interleaved scan of all components; 1 component, or 3 (YCbCr:
 * a JFIF APP0 or component ids 1, 2, 3) with chroma 1x1 and luma 1x1 (4:4:4), 2x1 (4:2:2) or 2x2 (4:2:0); 8-bit quantisation tables, at most
 * two DC and two AC Huffman tables, any number of DQT / DHT segments; DRI with any interval; APPn / COM skipped.  Not taken (cs_jpeg_probe
 * says CS_ERR_UNSUPPORTED and the caller decodes the file elsewhere): every other SOFn, 4 components, 12-bit, other samplings, a file with an
 * Adobe APP14 segment, subsampled files with W <= 4 (libjpeg's replication upsampler).  No equality with PIL is claimed for hand-made
 * coefficient blocks whose IDCT leaves the sample range by more than a few hundred; such files stay memory-safe and deterministic.
 * cs_jpeg_probe is host arithmetic over the file's bytes (no device is touched): the marker segments within n up to SOS.  CS_ERR_BAD_ARG for
 * framing that runs past n; it never reads at or beyond file + n.
 * cs_op_jpeg_decode: files is ONE device buffer of total_file_bytes bytes holding the files back to back, file i at file_offsets[i],
 * file_lengths[i] long (all arrays in device memory).  Sampling is per file: the kernel reads the headers itself and trusts nothing the host
 * said.  Three launches on `stream`, whatever I is; the call does not wait for the device.  status[i] (device) is 0 for a complete image or
 * one of CS_JPGDEC_*; a file with a non-zero status has written no pixel and has not disturbed the other files of the call.  Bytes behind the
 * last MCU are not examined.  workspace: device, 16-byte aligned, cs_jpeg_decode_workspace_bytes(...) bytes (host arithmetic; 0 for sizes the
 * decoder does not take).  1 <= H, W <= 4096 (CS_ERR_UNSUPPORTED above), 1 <= I <= 65535. */
enum { CS_JPEG_GRAY = 0, CS_JPEG_444 = 1, CS_JPEG_422 = 2, CS_JPEG_420 = 3 };
typedef struct cs_jpeg_info {
  int width, height, components;
  int sampling;          /* CS_JPEG_*, -1 when the decoder does not take the file */
  int restart_interval;  /* MCUs between restart markers, 0 without DRI */
  unsigned long long entropy_offset; /* first byte behind the SOS segment */
} cs_jpeg_info;
enum {
  CS_JPGDEC_OK = 0,
  CS_JPGDEC_BAD_FRAMING = 1,     /* SOI, a segment length past the file, no SOF / SOS */
  CS_JPGDEC_HEADER_MISMATCH = 2, /* SOF is not the call's H, W (or a form the decoder does not take) */
  CS_JPGDEC_BAD_TABLE = 3,       /* DHT with more codes than a length allows, more than 256 symbols or counts past the segment; a DQT
                                    index or precision; a table that a component selects but no segment defined */
  CS_JPGDEC_BAD_CODE = 4,        /* 16 bits that are no code of the table */
  CS_JPGDEC_BAD_SYMBOL = 5,      /* DC category above 11, AC size above 10, or a run past coefficient 63 */
  CS_JPGDEC_INPUT_EXHAUSTED = 6, /* the entropy data ends, or a marker other than the expected one appears, before the last MCU */
  CS_JPGDEC_BAD_RESTART = 7      /* a missing, misnumbered or surplus RSTn */
};
int cs_jpeg_probe(const uint8_t* file, size_t n, cs_jpeg_info* info);
size_t cs_jpeg_decode_workspace_bytes(int I, int H, int W, size_t total_file_bytes);
int cs_op_jpeg_decode(const uint8_t* files, const uint64_t* file_offsets, const uint32_t* file_lengths, size_t total_file_bytes, int I, int H,
                      int W, void* pixels, long long image_stride_bytes, uint32_t* status, void* workspace, cs_stream stream);
/* Progressive JPEG files on the device (csrc/jpegprog.hip): the _ex forms of the three entry points above.  With
 * flags = 0 each is the plain entry point: same results, statuses and error texts.  CS_JPEG_PROGRESSIVE adds SOF2 files:
 * cs_jpeg_probe_ex walks such a file to its EOI and takes it when the frame-level rules above hold, it has at most 32 scans, no DQT / DRI
 * behind the first SOS, every scan is legal by T.81 G.1.1.1.1 (a DC scan has Ss = Se = 0 and a subset of the components in frame order; an AC
 * scan one component and 1 <= Ss <= Se <= 63; Al <= 13; Ah = 0, or Ah = Al + 1 and equal to the Al the coefficients were last coded with; no
 * coefficient first-coded twice; AC behind the component's first DC scan -- what libjpeg only warns about is refused) and the progression is
 * complete: at EOI every coefficient of every component is coded down to bit 0 (an incomplete file is where libjpeg's block smoothing starts,
 * which is not built).  Anything else is CS_ERR_UNSUPPORTED with the reason; framing past n is CS_ERR_BAD_ARG.  `scans` (may be NULL) receives
 * the process, the number of scans (1 for a baseline file) and the offset of the first scan's data.
 * cs_op_jpeg_decode_ex with CS_JPEG_PROGRESSIVE takes baseline and progressive files of one (H, W) mixed in any order: four launches, whatever
 * I is (the baseline entropy kernel, the progressive one -- each leaves the files of the other process at once --, then the IDCT and the pixel
 * kernel once for the call); nothing waits for the device.  The contract is cs_op_jpeg_decode's: PIL's pixels exactly, or a status word and no
 * pixel, and a bad file does not disturb its neighbours.  The progressive kernel walks every segment again and re-checks every rule of the
 * probe; a violation is CS_JPGDEC_BAD_SCAN (8; a macro, the seven codes of the enum above keep their meaning).  The workspace is
 * cs_jpeg_decode_workspace_bytes_ex(..., flags) bytes: with the flag it also holds one restart table per scan, sized from H, W, I alone.
 * cs_debug_jpeg_scan_levels(0) makes the progressive kernel run one scan per level instead of its dependency levels (1, the default, restores
 * them): process-wide, for tests and tools that compare the two orders; the bits are the same. */
#define CS_JPEG_PROGRESSIVE 1
#define CS_JPGDEC_BAD_SCAN 8 /* an illegal or a 33rd scan, DQT / DRI behind the first SOS, or an incomplete progression */
typedef struct cs_jpeg_scan_info {
  int process; /* 0 baseline, 1 progressive */
  int scans;
  unsigned long long entropy_offset; /* the first scan's data */
} cs_jpeg_scan_info;
int cs_jpeg_probe_ex(const uint8_t* file, size_t n, int flags, cs_jpeg_info* info, cs_jpeg_scan_info* scans);
size_t cs_jpeg_decode_workspace_bytes_ex(int I, int H, int W, size_t total_file_bytes, int flags);
int cs_op_jpeg_decode_ex(const uint8_t* files, const uint64_t* file_offsets, const uint32_t* file_lengths, size_t total_file_bytes, int I, int H,
                         int W, void* pixels, long long image_stride_bytes, uint32_t* status, void* workspace, int flags, cs_stream stream);
void cs_debug_jpeg_scan_levels(int on);
/* de_norm_img + u8 (utils/misc/image.py:25-34, utils/io/images.py:20-23; batch_writer.py:117-135): I processed images fp32 CHW -> uint8 HWC,
 * x * std, then + mean, then * 255, each rounded on its own (no fma), truncated.  Values are clamped to [0, 255] first (NaN -> 0): that agrees
 * with the host form (a C cast) on every value the input stage produces (u8 / 255 normalised and de-normalised stays inside [0, 255]); outside
 * that range the host cast is undefined.  mean3 / std3 are HOST pointers. */
int cs_op_denorm_to_rgb8(const float* chw, int I, int H, int W, const float* mean3, const float* std3, uint8_t* out, cs_stream stream);
/* Test phase (task/test.py): the ground-truth side of the loss.
 * GT input stage: B device uint16 metric maps of one size (decoded 16-bit PNGs; rows in_row_elems samples apart, maps in_h * in_row_elems
 * apart) -> fp32 [B][out_h][out_w], the maps NvsDataset compares the score maps with.  load_content (nvs_dataset.py:429-457,
 * utils/io/images.py:32-46) first, in one of the modes below: SSIM_M1_1 m / 32767 - 1, SSIM_0_1 the same clamped to [0, 1], MAE m / 65535,
 * MSE the MAE value squared; then the antialiased bilinear resize to (rs_h, rs_w) of cs_op_preprocess_u8 (skipped when equal to the input
 * size) and the crop window (resize_all, nvs_dataset.py:218-241).  IEEE divisions: without a resize the output is bit-identical to the
 * reference's map.  maps == NULL gives B "empty_image" placeholders (nvs_dataset.py:441-454): 0 for the SSIM modes, NaN for MAE / MSE,
 * nothing is read.  1 <= B <= 1024.  scratch (device, B * in_h * rs_w floats) only when resizing; the filter tables are the image stage's
 * cache. */
enum { CS_METRIC_SSIM_M1_1 = 0, CS_METRIC_SSIM_0_1 = 1, CS_METRIC_MAE = 2, CS_METRIC_MSE = 3 };
int cs_op_metric_map_u16(const uint16_t* maps, int B, int in_h, int in_w, int in_row_elems, int mode, int rs_h, int rs_w, int crop_y, int crop_x,
                         int out_h, int out_w, float* out, float* scratch, cs_stream stream);
/* Ground-truth metric maps from the images themselves (csrc/gtmap.hip; DESIGN.md section 6, row f6: the reference ships no program that writes
 * its metric_map/ files, so this build owns the definition).  B pairs (render, captured image of the same view) of one size, device uint8 HWC
 * RGB with contiguous rows, images image_stride_bytes apart in both arrays -> B uint16 maps [B][H][out_row_elems], the layout
 * cs_op_metric_map_u16 takes as maps / in_row_elems and, with out_row_elems == W, cs_op_png_encode as CS_PNG_GRAY16.
 * CS_GTMAP_SSIM: pixels x / 255; 11 x 11 Gaussian window, sigma 1.5, sum 1; "same" size with zero padding (a pixel outside the image is 0 and
 * keeps its weight, F.conv2d(padding=5)); per channel ((2 mu_a mu_b + C1)(2 s_ab + C2)) / ((mu_a^2 + mu_b^2 + C1)(s_aa + s_bb + C2)), C1 = 0.01^2,
 * C2 = 0.03^2; the mean of the three channels m is stored as trunc((m + 1) * 32767) (metric_map_write for [-1, 1], utils/io/images.py:49-63).
 * fp32 on pixels shifted by a per-tile integer, which removes the cancellation of G*(a*a) - mu_a^2: identical images give 65534 everywhere.
 * CS_GTMAP_MAE (also the source of MSE): s = sum_c |a_c - b_c|, code (257 * s) / 3 = trunc(65535 * s / 765), integers only.
 * One launch for the batch, queued on `stream`; nothing is waited for or allocated.  1 <= B <= 1024, 1 <= H, W <= 65535 (CS_ERR_UNSUPPORTED
 * above); images smaller than the window are legal.  Bad arguments are rejected before anything is launched.  A map's codes depend on its own
 * pixel pair alone: the same bits alone and at any position of any batch. */
enum { CS_GTMAP_SSIM = 0, CS_GTMAP_MAE = 1 };
int cs_op_gt_metric_map_u8(const uint8_t* render, const uint8_t* gt, int B, int H, int W, long long image_stride_bytes, int kind,
                           uint16_t* out, int out_row_elems, cs_stream stream);
/* Per-frame sums of the ground-truth maps, the device side of the ground-truth score summary (crossscore_amd/summarise_gt.py; DESIGN.md
 * section 6, row f8).  Over a frame's n = H * W pairs of 16-bit samples (c_ssim from metric_map/ssim, c_mae from metric_map/mae):
 *   sums[b][0] = S1 = sum c_ssim
 *   sums[b][1] = S2 = sum min(max(c_ssim, 32767), 65534)   the clip of c / 32767 - 1 to [0, 1]: below 32767 reads negative, 65535 as 1.00003
 *   sums[b][2] = S3 = sum c_mae
 *   sums[b][3] = S4 = sum c_mae^2                          <= 65535^2 * 65535^2 < 2^64
 * unsigned 64-bit integers, exact; nothing is formed in floating point on the device.  The host forms (score_summariser.py:33-53)
 *   ssim_-1_1 = S1 / (32767 n) - 1, ssim_0_1 = (S2 - 32767 n) / (32767 n), mae = S3 / (65535 n), mse = S4 / (65535^2 n), psnr = -10 log10(mse).
 * Integer addition is associative: a frame's sums are the same numbers alone and at any position of any batch, whatever the order of tiles
 * and atomics.  Both ops zero `sums` (device, B * 4 words, 8-byte aligned) on `stream` and then queue one launch; nothing is waited for or
 * allocated.  1 <= B <= 1024, 1 <= H, W <= 65535 (CS_ERR_UNSUPPORTED above); bad arguments are rejected before anything is queued.
 * cs_op_metric_map_sums_u16: the maps as stored, two arrays [B][H][row_elems] of uint16 (2-byte aligned at least), row_elems >= W, frames
 * image_stride_elems >= (H - 1) * row_elems + W samples apart in both; only [row, row + W) of a row is read.
 * cs_op_gt_metric_sums_u8: the same four sums of the maps cs_op_gt_metric_map_u8 would write for the B pairs (CS_GTMAP_SSIM and CS_GTMAP_MAE,
 * same arguments), exactly, in one launch and without the maps in memory. */
int cs_op_metric_map_sums_u16(const uint16_t* ssim, const uint16_t* mae, int B, int H, int W, int row_elems, long long image_stride_elems,
                              uint64_t* sums, cs_stream stream);
int cs_op_gt_metric_sums_u8(const uint8_t* render, const uint8_t* gt, int B, int H, int W, long long image_stride_bytes, uint64_t* sums,
                            cs_stream stream);
/* Score-vs-GT sums: score, gt (B, H, W) fp32 -> stats (B, 6) fp64 = per image sum|s-g|, sum s, sum g, sum s^2, sum g^2, sum s*g, accumulated
 * in fp64 (the L1 loss, Pearson correlation and PSNR of task/core.py:265-293, 379-417 follow on the host).  Two launches, a fixed order: an
 * image's six sums have the same bits alone and at any position of any batch.  NaN propagates.  scratch: device, at least
 * cs_score_gt_workspace_bytes(B, H, W) bytes. */
size_t cs_score_gt_workspace_bytes(int B, int H, int W);
int cs_op_score_gt_stats(const float* score, const float* gt, int B, int H, int W, double* stats, void* scratch, cs_stream stream);
/* Score pooling: order statistics, worst-tail sums and the worst window of a batch of maps (crossscore_amd/pooling.py; DESIGN.md section 6, row
 * f13).  A map is H x W codes c in [0, 65535], n = H * W.  cs_op_score_pool_u16: the codes are the samples of B uint16 maps [B][H][row_elems],
 * row_elems >= W, maps image_stride_elems >= (H - 1) * row_elems + W samples apart; only [row, row + W) of a row is read.
 * cs_op_score_pool_f32: B contiguous fp32 maps; a pixel's code is exactly what cs_op_score_to_gray16 stores for it with the same signed_range
 * (m * 65535, or (m + 1) * 32767, truncated and clipped; NaN, +-Inf, -0.0 and values outside the range included: one device function).
 * With s[0] <= ... <= s[n - 1] the sorted codes and `permille` a HOST array of Q values q_j in [0, 1000] (1 <= Q <= 16, any order, duplicates
 * allowed), per map b:
 *   sum[b]       = sum c                                                       (u64)
 *   quant[b][j]  = s[(q_j * (n - 1)) / 1000]   integer division in 64 bits     (u32; q = 0 the minimum, 1000 the maximum, 500 the lower median)
 *   tail[b][j]   = sum of s[i], i < k_j,  k_j = max(1, (q_j * n) / 1000)       (u64; the k_j worst pixels; q = 1000 gives sum)
 *   window[b][0] = the smallest sum of codes over all S x S windows lying fully inside the map (1 <= S <= min(H, W, 255): below 2^32),
 *   window[b][1], window[b][2] = the y, x of its top-left corner; ties go to the smallest y, then the smallest x          (u64 each)
 * unsigned integers, exact; nothing is formed in floating point on the device.  The host forms values in the units of the written 16-bit map,
 * v = c / 65535 (signed_range 0) or c / 32767 - 1 (signed_range 1): a quantile v(quant), a tail mean v(tail / k), the window mean
 * v(window[0] / S^2), the 16-bit mean v(sum / n).  Integer addition and min on the packed (sum, y, x) key are associative: a map's words are the
 * same alone and at any position of any batch, whatever the order of tiles and atomics.
 * window == NULL or S == 0 skips the window launches.  Both ops initialise what they accumulate into on `stream` and queue their launches there;
 * nothing is waited for or allocated.  1 <= B <= 1024, 1 <= H, W <= 4096 (CS_ERR_UNSUPPORTED above).  S > min(H, W), S > 255, Q outside
 * [1, 16], a permille outside [0, 1000], a null required pointer and row_elems < W are CS_ERR_BAD_ARG, rejected before anything is queued.
 * sum, tail, window: device, 8-byte aligned; quant: 4-byte aligned; scratch: device, 16-byte aligned, at least
 * cs_score_pool_workspace_bytes(B, H, W, Q) bytes (host arithmetic; 0 for sizes the ops do not take). */
size_t cs_score_pool_workspace_bytes(int B, int H, int W, int Q);
int cs_op_score_pool_f32(const float* score, int B, int H, int W, int signed_range, const int32_t* permille, int Q, int S, uint64_t* sum,
                         uint32_t* quant, uint64_t* tail, uint64_t* window, void* scratch, cs_stream stream);
int cs_op_score_pool_u16(const uint16_t* codes, int B, int H, int W, int row_elems, long long image_stride_elems, const int32_t* permille, int Q,
                         int S, uint64_t* sum, uint32_t* quant, uint64_t* tail, uint64_t* window, void* scratch, cs_stream stream);
/* Preview sheet: up to CS_SHEET_MAX_PANELS panels painted into one (canvas_h, canvas_w, 3) uint8 canvas, in one launch (crossscore_amd/vis.py;
 * DESIGN.md section 6, row f14).  `panels` is a HOST array: its entries travel as kernel arguments, nothing is uploaded, waited for or allocated.
 * Panels are painted in array order, a later one covers an earlier one; a canvas pixel no panel covers is (0, 0, 0); every canvas byte is stored
 * exactly once and nothing else is.  Integer arithmetic throughout.  A panel's rectangle (dst_y, dst_x, dst_h, dst_w) lies inside the canvas; r, c
 * below are a pixel's row and column inside it.
 *   CS_SHEET_FILL   the rectangle takes rgb.
 *   CS_SHEET_IMAGE  exact area resampling of src (src_h x src_w uint8 HWC RGB, rows src_row_bytes >= 3 src_w apart) into dst_h x dst_w: with
 *                   sh, sw, dh, dw the four sizes, wx[i][j] = max(0, min((i + 1) dw, (j + 1) sw) - max(i dw, j sw)) and wy likewise with the
 *                   heights, per channel S = sum_iy sum_ix wy[iy][r] wx[ix][c] v[iy][ix] and out = (S + (sh sw) / 2) / (sh sw), integer
 *                   division (S < 2^32).  Equal sizes copy, an integer factor gives the rounded box mean, enlarging is allowed.
 *   CS_SHEET_BLEND  the same resampling of the image (a + b + 1) >> 1, formed per source pixel: a = src, b = src2 (src2_h x src2_w equal to
 *                   src_h x src_w, rows src2_row_bytes apart).
 *   CS_SHEET_RAMP   src is a 256 x 3 byte table; row r takes its entry 255 - (r 256) / dst_h.
 *   CS_SHEET_FRAME  the pixels with r < param, r >= dst_h - param, c < param or c >= dst_w - param take rgb (param >= 1: the outline, param
 *                   pixels thick on the inside); the others are untouched.
 *   CS_SHEET_TEXT   text: n = 1 .. 16 characters of "0123456789.- " (up to the first NUL) in a 5 x 7 font scaled by param >= 1
 *                   (csrc/sheet_font.h): the pixel takes rgb where bit 4 - gx of row gy of the glyph of character c / (6 param) is set, with
 *                   gx = (c mod 6 param) / param < 5 and gy = r / param; the others are untouched.  The rectangle is 7 param x (6 n - 1) param.
 * CS_ERR_BAD_ARG: a NULL canvas or panel array, an unknown kind, an empty rectangle or one outside the canvas, a NULL source where the kind reads
 * one, src_row_bytes < 3 src_w, unequal BLEND sources, param < 1, a TEXT rectangle of another size, no or an unknown character.
 * CS_ERR_UNSUPPORTED: more than CS_SHEET_MAX_PANELS panels, a canvas, rectangle or source side above CS_SHEET_MAX_SIDE.  Both before any launch. */
enum { CS_SHEET_FILL = 0, CS_SHEET_IMAGE = 1, CS_SHEET_BLEND = 2, CS_SHEET_RAMP = 3, CS_SHEET_FRAME = 4, CS_SHEET_TEXT = 5 };
enum { CS_SHEET_MAX_PANELS = 48, CS_SHEET_MAX_SIDE = 4096 };
typedef struct {
  int kind;
  int dst_y, dst_x, dst_h, dst_w;
  const uint8_t* src; /* device */
  int src_h, src_w, src_row_bytes;
  const uint8_t* src2; /* device */
  int src2_h, src2_w, src2_row_bytes;
  uint8_t rgb[3];
  int param;
  char text[16];
} cs_sheet_panel;
int cs_op_sheet_compose(const cs_sheet_panel* panels, int n_panels, uint8_t* canvas, int canvas_h, int canvas_w, cs_stream stream);
int cs_op_pos_bicubic(const float* pos, int G, int C, int gh, int gw, float* out, cs_stream stream);
/* the same with the resize convention as an argument: legacy = 0 F.interpolate(size=(gh, gw)) (cs_op_pos_bicubic), 1 the reference's pinned
 * transformers 4.33.3 form scale_factor=((gh + 0.1) / G, (gw + 0.1) / G) (cs_config.pos_interp_legacy; golden tests/golden/g6_pos_legacy.npz) */
int cs_op_pos_bicubic_ex(const float* pos, int G, int C, int gh, int gw, int legacy, float* out, cs_stream stream);
int cs_op_pe_bilinear(const float* pe, int ph, int pw, int C, int gh, int gw, float* out, cs_stream stream);
/* the same resize with the mode as an argument: 0 bilinear (cs_op_pe_bilinear), 1 bicubic; align_corners=True in both (cs_config.pe_interp_mode) */
int cs_op_pe_interp(const float* pe, int ph, int pw, int C, int gh, int gw, int mode, float* out, cs_stream stream);
/* fp32 [rows][K] -> fp16 [rows][ldo] (zero padded); row_scale (rows) / col_scale (K) may be NULL: LayerScale folded into the
 * rows of a projection, LayerNorm gamma into its columns */
/* 1 in *overlap when kernels queued on the two streams run side by side, 0 when the runtime serialises them (streams that share a
 * hardware queue, or hardware queues that share a dispatch pipe: a large grid on `a` then holds back a kernel on `b`).  Runs a two-round
 * grid of idle workgroups on `a` beside one idle wave on `b` and waits for them (~0.4 ms): a set-up helper, not for hot loops. */
int cs_op_streams_overlap(cs_stream a, cs_stream b, int* overlap);
int cs_op_pack_f16(const float* w, int rows, int K, uint16_t* out, int ldo, const float* row_scale, const float* col_scale,
                    cs_stream stream);
/* LayerNorm fold constants of a projection: s[n] = sum_k packed W'[n][k], c[n] = bias[n] + sum_k beta[k] W[n][k] */
int cs_op_ln_fold_consts(const uint16_t* w_packed, int ldp, const float* w, const float* beta, const float* bias, int N, int K,
                         float* s_out, float* c_out, cs_stream stream);
/* Encoder token-panel kernel (csrc/panel.hip; hidden 384, MLP 1536 only).  cs_op_panel_pack builds the weight stream the kernel
 * consumes from fp32 matrices: wo (C,C) [NULL: no out-projection units] with per-row scale ls1 (layer_scale1), w1 (4C,C) with
 * per-column scale g2 (norm2 gamma), w2 (C,4C) with per-row scale ls2 (layer_scale2); scales may be NULL.  img must hold
 * cs_panel_image_bytes(wo != NULL) bytes.  cs_op_encoder_panel then computes, in place on x (M,C) fp32,
 *   x += attn_o Wo'^T + bo   (skipped when attn_o is NULL);   x += GELU(norm(x) W1'^T + b1) W2'^T + b2;
 *   u_out = fp16(norm(x))    (skipped when NULL), norm = LayerNorm without gamma/beta (HF modeling_dinov2.py:361-380). */
/* debug switch, process-wide (see cs_debug_* above): which of the two token-panel kernels handles created from now on (their weight images are
 * packed in cs_finalize) and the cs_op_panel_* entry points use: 0 = csrc/panel.hip (8 waves in role-split pairs, rounds 2-5), 1 = csrc/panel4.hip
 * (4 waves, one per SIMD, column-split residual products; round 6).  The images differ: pack and launch under the same setting. */
void cs_debug_panel_impl(int impl);
int cs_panel_supported(int hidden, int mlp_ratio);
size_t cs_panel_image_bytes(int with_outproj);
int cs_op_panel_pack(const float* wo, const float* ls1, const float* w1, const float* g2, const float* w2, const float* ls2,
                     uint16_t* img, cs_stream stream);
int cs_op_encoder_panel(float* x, const uint16_t* attn_o, const uint16_t* img, const float* bo, const float* b1, const float* b2,
                        uint16_t* u_out, int M, float eps, cs_stream stream);
/* debug switch, process-wide (see cs_debug_* above).  Kernel selection of cs_op_gemm / the forward's linears: 1 (default) = shapes with K >= 384, N a multiple of
 * 256 and M >= 256 run on the 256 x 256 x 64-tile kernel (csrc/gemm256.hip), everything else on the 128-row kernel (csrc/gemm.hip);
 * 0 = the 128-row kernel for every shape (a wide backbone's LayerNorm-folded chunks, whose epilogues exist only in the 256-tile kernel, then run
 * LayerNorm launches + the 128-row kernel's plain epilogues: cs_forward asks cs_gemm256_supported per chunk).  The two kernels add the same products
 * in the same order: their results are bit-identical (tested). */
void cs_debug_gemm256_enable(int on);
/* debug switch, process-wide: the smallest K the 256-tile kernel takes (default 384; tools/qkv_k384_try.py compares 384 with 512) */
void cs_debug_gemm256_kmin(int k);
/* debug switch, process-wide, read at every launch (single ops and whole forwards alike): the block count of the persistent grids of both GEMM
 * kernels in place of the CU-derived one (2 x CUs for the 128-row kernel, 1 x CUs for the 256-tile kernel).  The launchers' clamps still apply:
 * rounded down to a multiple of 8, at most one block per tile of the fullest XCD, at least 8.  0 (the default) = from the CU count.  With 8 blocks
 * each XCD's single block walks all of its tiles; with 16 two blocks of an XCD interleave.  The results do not depend on it (tested). */
void cs_debug_gemm_grid(int blocks);
/* The decoder's sub-block closing  x = LN(x + Linear(y))  (model/customised_transformer/transformer.py:157-173) in one launch (csrc/rowln.hip;
 * K = N = C = 384: the ViT-S decoder): out_f32 / out_f16 (M, C) = LayerNorm(resid + A W^T + bias; gamma, beta, eps); resid may be NULL
 * (decoder_do_short_cut off) and may alias out_f32.  CS_ERR_BAD_ARG for other widths (the forward then runs GEMM + LayerNorm).
 * cs_debug_rowln_enable(0): process-wide debug switch back to the two-launch form (see cs_debug_* above). */
int cs_op_linear_layernorm(const uint16_t* A, const uint16_t* W, const float* bias, const float* resid, const float* gamma, const float* beta,
                           float eps, float* out_f32, uint16_t* out_f16, int M, int C, cs_stream stream);
/* ... and with the sub-block's NEXT linear in the same launch (the forward's default where C = 384 for the C-wide ones: the cross-attention's
 * Q projection behind norm1, linear1 + ReLU behind norm2, the head's first linear + LeakyReLU behind the last norm3; the 3 C-wide form, the next
 * layer's packed QKV projection, is built and tested but measured slower than a GEMM of its own, so the forward does not use it;
 * transformer.py:157-173,182-210, cross_reference.py:45-50): out2 (M, n2) = act2(LN rows, rounded to the operand type, x W2 (n2, C)^T + bias2),
 * n2 = C or 3 C, act2 0 none / 1 ReLU / 2 LeakyReLU(0.01).  out_f32 / out_f16 may be NULL when only out2 is wanted; out2 may alias A (a
 * workgroup writes the 64 rows it read at its start). */
int cs_op_linear_layernorm_linear(const uint16_t* A, const uint16_t* W, const float* bias, const float* resid, const float* gamma,
                                  const float* beta, float eps, float* out_f32, uint16_t* out_f16, const uint16_t* W2, const float* bias2,
                                  int n2, int act2, uint16_t* out2, int M, int C, cs_stream stream);
/* 1 (default): both fusions; 2: linear + LayerNorm in one launch, the next linear as a GEMM of its own; 0: GEMM + LayerNorm + GEMM */
void cs_debug_rowln_enable(int on);
/* number of column tiles the GEMM launcher uses for N output columns (LayerNorm partial-sum slots per row = 4 x this) */
int cs_gemm_column_tiles(int N);

/* ---- Fitting the regression head on the device (csrc/headfit.hip) ----
 * The head is ref_cross.head.{0,2}: Linear(C, C) "a" -> LeakyReLU(0.01) -> Linear(C, P P) "b" -> sigmoid | tanh -> pow -> jigsaw.  X (M, C) are
 * the 16-bit tokens behind the last norm3, A (M, C) the 16-bit hidden rows, M = B gh gw.  Loss = inv_count * sum |s - gt|; the gradient g of
 * the sum with respect to z = A Wb^T + bb is rounded once to the operand type, dpre = (g Wb) * (A > 0 ? 1 : 0.01) once more; the four
 * gradients are fp32 and carry the factor inv_count, applied in fp32 behind each reduction (no loss scaling is needed).  Every sum over rows has
 * a fixed order and there are no atomics: two runs give the same bits.  Operand type of the cs_op_* forms: cs_debug_set_op_operand_dtype.
 * Every entry rejects null or misaligned pointers (16-bit operands: 16 bytes, row strides multiples of 8 elements; fp32: 4 bytes; the loss: 8)
 * and unsupported shapes before any launch; workspaces are device memory, 256-byte aligned. */
/* widths the kernels take: hidden a multiple of 64 in [64, 4096] (every width the forward's head GEMM takes), patch 14 */
int cs_head_fit_supported(int hidden, int patch);
/* tile sizes the tests place their edge cases by: rows per workgroup of cs_op_head_grad_z, rows per fp32 partial of cs_op_gemm_tn, and the columns
 * of g (P P = 196 padded to whole 32-deep k steps) */
int cs_head_fit_row_tile(void);
int cs_head_fit_row_chunk(void);
int cs_head_fit_g_columns(void);
/* bytes of `ws` for cs_op_head_backward (and for cs_op_head_grad_z with the same M) */
size_t cs_head_backward_workspace_bytes(int M, int C, int P);
/* bytes of `ws` for cs_op_gemm_tn */
size_t cs_gemm_tn_workspace_bytes(int M, int N, int K);
/* g (M, ldg >= cs_head_fit_g_columns()) = sign(s - gt) ds/dz with zeros in columns 196 .. 223; *loss_sum += sum |s - gt| (fp32 terms, summed in
 * fp64); colsum_part (may be NULL): (ceil(M / row tile), cs_head_fit_g_columns()) per-workgroup column sums of the rounded g.  act 0 sigmoid, 1 tanh
 * (tanh with powp != 1 is CS_ERR_UNSUPPORTED in every head-fit entry: the reference forces p = 1 there). */
int cs_op_head_grad_z(const uint16_t* A, int lda, const uint16_t* Wb, int ldw, const float* bb, const float* gt, int B, int gh, int gw, int P, int C,
                      int act, float powp, uint16_t* g, int ldg, double* loss_sum, float* colsum_part, void* ws, cs_stream stream);
/* debug (tests): cs_op_head_grad_z that also stores s (M, P P) fp32 as its epilogue formed it into s_out (required); per call, no state */
int cs_debug_op_head_grad_z_tap(const uint16_t* A, int lda, const uint16_t* Wb, int ldw, const float* bb, const float* gt, int B, int gh, int gw, int P,
                                int C, int act, float powp, uint16_t* g, int ldg, double* loss_sum, float* colsum_part, float* s_out, void* ws,
                                cs_stream stream);
/* out (N, K; rows ldo apart) = (accumulate ? out : 0) + scale * sum_m G[m][n] X[m][k]; colsum (NULL or N) the same for sum_m G[m][n].  K a multiple of 8. */
int cs_op_gemm_tn(const uint16_t* G, int ldg, const uint16_t* X, int ldx, int M, int N, int K, float scale, int accumulate, float* out, int ldo,
                  float* colsum, void* ws, cs_stream stream);
/* the whole backward: dWa (C, C), dba (C), dWb (P P, C), dbb (P P), *loss (device), each = (accumulate ? itself : 0) + inv_count * its sum */
int cs_op_head_backward(const uint16_t* X, int ldx, const uint16_t* A, int lda, const uint16_t* Wb, int ldw, const float* bb, const float* gt, int B,
                        int gh, int gw, int P, int C, int act, float powp, double inv_count, int accumulate, float* dWa, float* dba, float* dWb,
                        float* dbb, double* loss, void* ws, cs_stream stream);
/* The same on the tokens and hidden rows the LAST cs_forward* call on this handle left in its workspace, with the handle's packed Wb, bias,
 * activation and power; gt (B, H, W) fp32.  CS_ERR_STATE if no forward ran, if it failed, if its (B, H, W) differ or if it only encoded
 * references.  inv_count and accumulate let sub-batches add up to one batch gradient.  Allocates its own workspace on first use. */
int cs_head_backward(cs_handle h, const float* gt, int B, int H, int W, double inv_count, int accumulate, float* dWa, float* dba, float* dWb,
                     float* dbb, double* loss, cs_stream stream);
/* debug: copies of the tokens X and hidden rows A (rows, C; 16 bit, contiguous) cs_head_backward would read; either may be NULL.  rows must be
 * the last forward's B Np (CS_ERR_BAD_ARG otherwise: nothing is copied). */
int cs_debug_head_inputs(cs_handle h, uint16_t* X, uint16_t* A, int rows, cs_stream stream);
/* torch.optim.AdamW's single-tensor step (amsgrad off) in place on fp32 p, m, v from g; step counts from 1; p16 (NULL or n): the updated
 * parameter rounded once to the operand type, in the same pass */
int cs_op_adamw(float* p, float* m, float* v, const float* g, long long n, float lr, float beta1, float beta2, float eps, float weight_decay,
                int step, uint16_t* p16, cs_stream stream);
/* Re-packs fp32 device weights (w0 (C, C), b0 (C), w2 (P P, C), b2 (P P)) into the finalised handle's existing head buffers, in stream order
 * behind the handle's last call; the handle is not rebuilt.  A forward queued on ANOTHER stream at the same time races with it: that is the
 * caller's to order. */
int cs_set_head_weights(cs_handle h, const float* w0, const float* b0, const float* w2, const float* b2, cs_stream stream);

/* ---- Fitting the decoder's tail with the head (csrc/tailfit.hip) ----
 * The tail is the last decoder layer's linear1 -> ReLU -> linear2 -> + residual -> norm3 and the head behind it: ten tensors.  x2 (M, C) fp32 is
 * that layer's norm2 output, H (M, C) 16 bit = relu(linear1(x2)) as the forward stored it.  The backward recomputes y = x2 + H W2^T + b2 in fp32
 * from the packed W2 (the forward never stores its pre-LayerNorm sum), takes mean, rstd and xhat from y two-pass in fp32, and forms
 *   dX = dpre Wa (fp32; dpre is the head backward's, 16 bit),  dgamma = inv_count sum_m dX xhat,  dbeta = inv_count sum_m dX,
 *   dy = rstd (gamma dX - mean_c(gamma dX) - xhat mean_c(gamma dX xhat)) rounded once to the operand type,  db2 = inv_count sum_m dy,
 *   dW2 = inv_count dy^T H,  dH = (dy W2) [H > 0] rounded once,  db1 = inv_count sum_m dH,  dW1 = inv_count dH^T x2 (x2 rounded once).
 * The gradient stops at x2.  W1, b1 and norm3's bias enter none of the ten gradients, so no entry takes them.  Sums over rows have a fixed order
 * and there are no atomics; pointer, stride and workspace rules are the head fit's, fp32 ROWS (x2, y, dX) and gamma are 16-byte aligned. */
/* the head's condition with hidden <= 2048, the widest LayerNorm the forward's decoder runs */
int cs_tail_fit_supported(int hidden, int patch);
/* rows per workgroup (= per fp32 partial of dgamma / dbeta) of cs_op_ln_backward, for the tests' edge cases */
int cs_tail_fit_ln_row_tile(void);
size_t cs_ln_backward_workspace_bytes(int M, int C);
size_t cs_tail_backward_workspace_bytes(int M, int C, int P);
/* LayerNorm backward on rows y (M, ldy) and dX (M, ldx) in fp32: dyh (M, ldd) 16 bit (bf16: 0 IEEE half, 1 bfloat16); dgamma, dbeta (C) =
 * (accumulate ? itself : 0) + inv_count * its sum.  C a multiple of 64 in [64, 2048]; row strides multiples of 4 elements. */
int cs_op_ln_backward(const float* y, int ldy, const float* dX, int ldx, const float* gamma, int M, int C, float eps, int bf16, float inv_count,
                      int accumulate, uint16_t* dyh, int ldd, float* dgamma, float* dbeta, void* ws, cs_stream stream);
/* the whole backward on caller-owned tensors: x2 contiguous; W2 (C, C), Wa (C, C), Wb (P P, C) packed 16 bit; the six tail gradients dW1 (C, C),
 * db1, dW2 (C, C), db2, dgamma3, dbeta3 (C) and the head's four, which are bit for bit cs_op_head_backward's on the same X, A, Wb, bb, gt */
int cs_op_tail_backward(const float* x2, const uint16_t* H, int ldh, const uint16_t* X, int ldx, const uint16_t* A, int lda, const uint16_t* W2,
                        int ldw2, const float* b2, const float* gamma3, float eps, const uint16_t* Wa, int ldwa, const uint16_t* Wb, int ldw,
                        const float* bb, const float* gt, int B, int gh, int gw, int P, int C, int act, float powp, double inv_count,
                        int accumulate, float* dW1, float* db1, float* dW2, float* db2, float* dgamma3, float* dbeta3, float* dWa, float* dba,
                        float* dWb, float* dbb, double* loss, void* ws, cs_stream stream);
/* A persistent switch like cs_debug_capture, off by default.  On: every cs_forward* call that runs the decoder also queues two stream-ordered
 * device-to-device copies (x2 and H, between the two closings of the last decoder layer) into a region the handle owns, allocated on first use;
 * the score map, the mean and every tap keep their bits.  Off: no launch, copy, allocation or byte of the forward changes. */
int cs_fit_tail_keep(cs_handle h, int on);
/* cs_op_tail_backward on what the LAST cs_forward* call on this handle left (with cs_fit_tail_keep on), with the handle's packed weights.
 * CS_ERR_STATE in the cases of cs_head_backward, and when that forward ran with the switch off. */
int cs_tail_backward(cs_handle h, const float* gt, int B, int H, int W, double inv_count, int accumulate, float* dW1, float* db1, float* dW2,
                     float* db2, float* dgamma3, float* dbeta3, float* dWa, float* dba, float* dWb, float* dbb, double* loss, cs_stream stream);
/* debug: copies of x2 (rows, C) fp32 and H (rows, C) 16 bit cs_tail_backward would read; either may be NULL; rows as in cs_debug_head_inputs */
int cs_debug_tail_inputs(cs_handle h, float* x2, uint16_t* H, int rows, cs_stream stream);
/* Re-packs fp32 device weights of the LAST decoder layer (linear1 and linear2 weight (C, C) and bias (C), norm3 weight and bias (C)) into the
 * finalised handle's existing buffers, in stream order behind the handle's last call; the race caveat of cs_set_head_weights holds. */
int cs_set_tail_weights(cs_handle h, const float* w1, const float* b1, const float* w2, const float* b2, const float* g3, const float* b3,
                        cs_stream stream);

/* ---- Attention backward (csrc/attnbwd.hip) ----
 * The backward of cs_op_attention on the same operands: Q, K, V, O and dO are 16 bit (cs_debug_set_op_operand_dtype), addressed as there (row
 * stride, batch stride, head hd at column hd * dh), lse (batch, heads, Lq) is what cs_op_attention wrote with the same q_scale.  Per batch item
 * and head, with Q' = Q (q_scale = 1: the producer folded the scale) or Q * q_scale rounded once (0 = log2(e)/sqrt(dh)), as the forward rounds it:
 *   S2 = Q' K^T,  P = 2^(S2 - lse),  D[q] = sum_d dO[q][d] O[q][d],  dP = dO V^T,  dz = P (dP - D)                    (all fp32)
 *   dV = Ph^T dO,  dK = dzh^T Q',  dQ = dzh K             (Ph, dzh: P and dz rounded once to the operand type; fp32 sums, rounded once on store)
 * dK and dQ are UNSCALED: the gradient with respect to K is ln2 * dK, the one with respect to Q' is ln2 * dQ; a consumer puts the scalar into
 * its own fp32 reduction.  P is recomputed and never stored; rows past Lq and keys past Lk are neither read nor written.  Three launches, no
 * atomics, every sum in a fixed order: two identical calls give identical bits.  dK and dV may sit side by side in one buffer.
 * CS_ERR_BAD_ARG before any launch: a null pointer, a 16-bit operand that is not 16-byte aligned, a workspace that is not 256-byte aligned, a row
 * or batch stride that is not a multiple of 8 elements, Lk * ldk (or * ldv, Lq * ldq, Lq * lddo) at or above 2^30.  CS_ERR_UNSUPPORTED: dh other
 * than 16, 48, 96.  ws: device memory of cs_attention_backward_workspace_bytes (0 for an unsupported shape). */
size_t cs_attention_backward_workspace_bytes(int batch, int heads, int Lq, int Lk, int dh);
/* the query rows a workgroup of the dQ kernel owns and the keys a workgroup of the dK / dV kernel owns (both also stream the other axis in tiles
 * of that size), for the tests' edge cases; CS_ERR_UNSUPPORTED for a head dim the backward is not built for */
int cs_attention_backward_tiles(int dh, int* q_tile, int* k_tile);
int cs_op_attention_backward(const uint16_t* Q, const uint16_t* K, const uint16_t* V, const uint16_t* O, const uint16_t* dO, const float* lse,
                             int ldq, int ldk, int ldv, int ldo, int lddo, long long q_bs, long long k_bs, long long v_bs, long long o_bs,
                             long long do_bs, int batch, int heads, int Lq, int Lk, int dh, float q_scale, uint16_t* dQ, int lddq,
                             long long dq_bs, uint16_t* dK, int lddk, long long dk_bs, uint16_t* dV, int lddv, long long dv_bs, void* ws,
                             cs_stream stream);

/* ---- Fitting the last decoder layer's cross-attention with the tail and the head (csrc/crossfit.hip) ----
 * Sixteen tensors: the layer's multihead_attn.in_proj_weight (3C, C) and in_proj_bias (3C), out_proj.weight (C, C) and bias (C), norm2 weight and
 * bias (C), and the tail's ten.  M = B Np query rows, Mk = M N memory rows, dh = C / heads.  x1 (M, C) fp32 is the row set that entered the block
 * (norm1's output, or the layer's input without self-attention); Q' (M, ldq) the 16-bit query projection as the forward stored it (log2(e)/sqrt(dh)
 * folded in); K, V the layer's column blocks of the packed K | V rows (Mk, ldkv); O (M, ldo) the attention output; lse (B, heads, Np) the kernel's;
 * mem (Mk, ldm) the reference tokens the K / V projection read.  The backward continues the tail's chain (whose ten gradients and loss come out
 * bit for bit as cs_op_tail_backward's):
 *   dx2 = f32(dyh) + dHh W1 (fp32),  y2 = (short_cut ? x1 : 0) + O Wo^T + bo recomputed in fp32,  (dgamma2, dbeta2, dy2h) = the LayerNorm backward
 *   dbo = inv_count sum_m dy2h,  dWo = inv_count dy2h^T O,  dOh = dy2h Wo rounded once,  (dQu, dKu, dV) = cs_op_attention_backward
 *   in_proj rows [0, C): inv_count / sqrt(dh) dQu^T x1h (x1 rounded once);  [C, 2C): inv_count ln2 dKu^T mem;  [2C, 3C): inv_count dV^T mem;
 *   in_proj_bias: the matching column sums (rows [C, 2C) are zero in exact arithmetic and carry rounding residue).
 * The gradient stops at x1 and at mem.  Fixed summation orders, no atomics.  Pointer, stride and workspace rules are the tail fit's. */
/* the tail's condition and a head dim the attention backward is built for (16, 48, 96) */
int cs_cross_fit_supported(int hidden, int heads, int patch);
size_t cs_cross_backward_workspace_bytes(int B, int Np, int N, int C, int P, int heads);
/* the whole backward on caller-owned tensors: x1 and x2 contiguous; W1, Wo, W2, Wa (C, C) and Wb (P P, C) packed 16 bit */
int cs_op_cross_backward(const float* x1, const uint16_t* Qp, int ldq, const uint16_t* K, const uint16_t* V, int ldkv, const uint16_t* O, int ldo,
                         const float* lse, const uint16_t* mem, int ldm, const uint16_t* W1, int ldw1, const uint16_t* Wo, int ldwo, const float* bo,
                         const float* gamma2, int N, int heads, int short_cut, const float* x2, const uint16_t* H, int ldh, const uint16_t* X,
                         int ldx, const uint16_t* A, int lda, const uint16_t* W2, int ldw2, const float* b2, const float* gamma3, float eps,
                         const uint16_t* Wa, int ldwa, const uint16_t* Wb, int ldw, const float* bb, const float* gt, int B, int gh, int gw, int P,
                         int C, int act, float powp, double inv_count, int accumulate, float* dWin, float* dbin, float* dWo, float* dbo,
                         float* dgamma2, float* dbeta2, float* dW1, float* db1, float* dW2, float* db2, float* dgamma3, float* dbeta3, float* dWa,
                         float* dba, float* dWb, float* dbb, double* loss, void* ws, cs_stream stream);
/* A persistent switch like cs_fit_tail_keep, off by default, and it implies that switch's two copies.  On: the last decoder layer's cross-attention
 * also writes its lse, and x1 is copied device-to-device on the forward's stream, in front of the norm2 closing that overwrites it, into a region
 * the handle owns (one more copy: cs_forward_stats counts cross_keep=1).  Q', the packed K | V rows and O are read from the workspace where the
 * forward left them (nothing behind that attention writes them), the reference tokens from the caller's ref_tokens (cached mode: keep them alive
 * until the backward has run) or from the workspace.  The score map, the mean and every tap keep their bits.  Off: nothing of the forward changes. */
int cs_fit_cross_keep(cs_handle h, int on);
/* cs_op_cross_backward on what the LAST cs_forward* call on this handle left (with cs_fit_cross_keep on), with the handle's packed weights.
 * CS_ERR_STATE in the cases of cs_tail_backward, and when that forward ran with cs_fit_cross_keep off. */
int cs_cross_backward(cs_handle h, const float* gt, int B, int H, int W, double inv_count, int accumulate, float* dWin, float* dbin, float* dWo,
                      float* dbo, float* dgamma2, float* dbeta2, float* dW1, float* db1, float* dW2, float* db2, float* dgamma3, float* dbeta3,
                      float* dWa, float* dba, float* dWb, float* dbb, double* loss, cs_stream stream);
/* debug: contiguous copies of x1 (rows, C) fp32, Q' and O (rows, C) 16 bit, lse (B, heads, Np) fp32 and the K and V rows (rows N, C) 16 bit that
 * cs_cross_backward would read; any may be NULL; rows as in cs_debug_head_inputs */
int cs_debug_cross_inputs(cs_handle h, float* x1, uint16_t* Qp, uint16_t* O, float* lse, uint16_t* K, uint16_t* V, int rows, cs_stream stream);
/* Re-packs fp32 device weights of the LAST decoder layer's cross-attention block (multihead_attn.in_proj_weight (3C, C) and in_proj_bias (3C),
 * out_proj weight (C, C) and bias (C), norm2 weight and bias (C)) into the finalised handle's existing buffers exactly as cs_finalize packs them
 * (the query rows with log2(e)/sqrt(dh) folded in), in stream order behind the handle's last call; the race caveat of cs_set_head_weights holds. */
int cs_set_cross_weights(cs_handle h, const float* in_proj_w, const float* in_proj_b, const float* out_w, const float* out_b, const float* g2,
                         const float* b2, cs_stream stream);

/* ---- Fitting the whole last decoder layer: its self-attention and norm1 with the cross-attention fit (csrc/layerfit.hip) ----
 * Twenty-two tensors: the layer's self_attn.in_proj_weight (3C, C) and in_proj_bias (3C), self_attn.out_proj.weight (C, C) and bias (C), norm1
 * weight and bias (C), and the cross-attention fit's sixteen.  x0 (M, C) fp32 is the row set that entered the layer; Qs', Ks, Vs the three C-wide
 * column blocks of the 16-bit packed projection rows (M, ldqkv) as the forward stored them (log2(e)/sqrt(dh) folded into Qs'); Os (M, ldos) the
 * self-attention's output and lse_s (B, heads, Np) its base-2 log-sum-exp; every batch item attends to its own Np rows.  Wq (C, C) is the
 * cross-attention's packed query projection (the scale folded in), Wo_s the self-attention's packed out_proj.  The backward continues the cross
 * fit's chain (whose sixteen gradients and loss come out bit for bit as cs_op_cross_backward's), with dQu that block's stored query gradient:
 *   dx1 = (short_cut ? f32(dy2h) : 0) + ln2 dQu Wq (fp32; the ln2 applied in fp32),  y1 = (short_cut ? x0 : 0) + Os Wo_s^T + bo_s recomputed in fp32,
 *   (dgamma1, dbeta1, dy1h) = the LayerNorm backward,  dbo_s = inv_count sum_m dy1h,  dWo_s = inv_count dy1h^T Os,  dOsh = dy1h Wo_s rounded once,
 *   (dQu_s, dKu_s, dV_s) = cs_op_attention_backward with Lq = Lk = Np,
 *   in_proj rows [0, C): inv_count / sqrt(dh) dQu_s^T x0h (x0 rounded once);  [C, 2C): inv_count ln2 dKu_s^T x0h;  [2C, 3C): inv_count dV_s^T x0h;
 *   in_proj_bias: the matching column sums.
 * The gradient stops at x0.  Fixed summation orders, no atomics.  Pointer, stride and workspace rules are the cross-attention fit's. */
/* the cross-attention fit's condition, and a decoder with self-attention */
int cs_layer_fit_supported(int hidden, int heads, int patch, int do_self_attn);
size_t cs_layer_backward_workspace_bytes(int B, int Np, int N, int C, int P, int heads);
/* the whole backward on caller-owned tensors: x0, x1 and x2 contiguous; Qs, Ks, Vs share the row pitch ldqkv; the weights packed 16 bit */
int cs_op_layer_backward(const float* x0, const uint16_t* Qs, const uint16_t* Ks, const uint16_t* Vs, int ldqkv, const uint16_t* Os, int ldos,
                         const float* lse_s, const uint16_t* Wq, int ldwq, const uint16_t* Wo_s, int ldwos, const float* bo_s, const float* gamma1,
                         const float* x1, const uint16_t* Qp, int ldq, const uint16_t* K, const uint16_t* V, int ldkv, const uint16_t* O, int ldo,
                         const float* lse, const uint16_t* mem, int ldm, const uint16_t* W1, int ldw1, const uint16_t* Wo, int ldwo, const float* bo,
                         const float* gamma2, int N, int heads, int short_cut, const float* x2, const uint16_t* H, int ldh, const uint16_t* X,
                         int ldx, const uint16_t* A, int lda, const uint16_t* W2, int ldw2, const float* b2, const float* gamma3, float eps,
                         const uint16_t* Wa, int ldwa, const uint16_t* Wb, int ldw, const float* bb, const float* gt, int B, int gh, int gw, int P,
                         int C, int act, float powp, double inv_count, int accumulate, float* dWin_s, float* dbin_s, float* dWo_s, float* dbo_s,
                         float* dgamma1, float* dbeta1, float* dWin, float* dbin, float* dWo, float* dbo, float* dgamma2, float* dbeta2, float* dW1,
                         float* db1, float* dW2, float* db2, float* dgamma3, float* dbeta3, float* dWa, float* dba, float* dWb, float* dbb,
                         double* loss, void* ws, cs_stream stream);
/* A persistent switch like cs_fit_cross_keep, off by default, and it implies that switch's copies.  On: the last decoder layer's self-attention also
 * writes its lse, straight into a region the handle owns, and x0 (in front of the norm1 closing that overwrites it) and Os (in front of the
 * cross-attention that overwrites it) are copied there device-to-device on the forward's stream (two more copies: cs_forward_stats counts
 * layer_keep=2).  The packed Q' | K | V rows are read from the workspace where the forward left them (nothing behind that attention writes them).
 * The score map, the mean and every tap keep their bits.  Off: nothing of the forward changes. */
int cs_fit_layer_keep(cs_handle h, int on);
/* cs_op_layer_backward on what the LAST cs_forward* call on this handle left (with cs_fit_layer_keep on), with the handle's packed weights.
 * CS_ERR_STATE in the cases of cs_cross_backward, and when that forward ran with cs_fit_layer_keep off; CS_ERR_UNSUPPORTED without self-attention. */
int cs_layer_backward(cs_handle h, const float* gt, int B, int H, int W, double inv_count, int accumulate, float* dWin_s, float* dbin_s, float* dWo_s,
                      float* dbo_s, float* dgamma1, float* dbeta1, float* dWin, float* dbin, float* dWo, float* dbo, float* dgamma2, float* dbeta2,
                      float* dW1, float* db1, float* dW2, float* db2, float* dgamma3, float* dbeta3, float* dWa, float* dba, float* dWb, float* dbb,
                      double* loss, cs_stream stream);
/* debug: contiguous copies of x0 (rows, C) fp32, Qs', Ks, Vs and Os (rows, C) 16 bit and lse_s (B, heads, Np) fp32 that cs_layer_backward would
 * read; any may be NULL; rows as in cs_debug_head_inputs */
int cs_debug_layer_inputs(cs_handle h, float* x0, uint16_t* Qs, uint16_t* Ks, uint16_t* Vs, uint16_t* Os, float* lse_s, int rows, cs_stream stream);
/* Re-packs fp32 device weights of the LAST decoder layer's self-attention block (self_attn.in_proj_weight (3C, C) and in_proj_bias (3C), out_proj
 * weight (C, C) and bias (C), norm1 weight and bias (C)) into the finalised handle's existing buffers exactly as cs_finalize packs them (the query
 * rows with log2(e)/sqrt(dh) folded in), in stream order behind the handle's last call; the race caveat of cs_set_head_weights holds. */
int cs_set_layer_weights(cs_handle h, const float* in_proj_w, const float* in_proj_b, const float* out_w, const float* out_b, const float* g1,
                         const float* b1, cs_stream stream);

#ifdef __cplusplus
}
#endif
#endif
