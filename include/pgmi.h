/*
 * pgmi.h -- C ABI of libpgmi, the MI355X-native (gfx950) PaliGemma-3B inference path.
 *
 * This is the drop-in boundary below the reference's Python API
 * (PaliGemmaForConditionalGeneration / SiglipVisionModel / GemmaForCausalLM / KVCache in
 * /root/reference/modeling_gemma.py and modeling_siglip.py).  The reference itself has no
 * FFI -- it is pure PyTorch -- so each entry point names the reference function whose body it
 * replaces; INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions
 *   - plain C, every call returns 0 on success or a negative PGMI_E* code; the message of the
 *     last failure on the calling thread is pgmi_last_error().
 *   - device pointers are HIP device memory of the context's device; streams are hipStream_t
 *     passed as void* (NULL = the default stream).  Calls are stream-ordered and do not
 *     synchronise unless stated.
 *   - bf16 tensors are raw uint16 bit patterns, row-major, contiguous.
 *   - one context per GPU; a context is not re-entrant (the reference is single-threaded).
 */
#ifndef PGMI_H
#define PGMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PGMI_OK 0
#define PGMI_E_ARG -1     /* ValueError in the Python layer   */
#define PGMI_E_STATE -2   /* AssertionError / misuse          */
#define PGMI_E_HIP -3     /* HIP runtime error                */
#define PGMI_E_NOMEM -4   /* allocation failure               */

#define PGMI_DTYPE_BF16 0
#define PGMI_DTYPE_F16 1
#define PGMI_DTYPE_F32 2

typedef struct pgmi_ctx pgmi_ctx;

/* Mirrors SiglipVisionConfig (modeling_siglip.py:7-34), GemmaConfig (modeling_gemma.py:39-71)
 * and PaliGemmaConfig (modeling_gemma.py:74-105), plus workspace capacities. */
typedef struct pgmi_config {
    int v_hidden, v_intermediate, v_layers, v_heads, v_channels, v_image, v_patch;
    float v_ln_eps;
    int t_vocab, t_hidden, t_intermediate, t_layers, t_heads, t_kv_heads, t_head_dim, t_max_pos;
    float t_rms_eps, t_rope_theta;
    int projection_dim;
    int64_t image_token_index;
    int64_t pad_token_id; /* -1 when the config's pad_token_id is None (modeling_gemma.py:453) */
    int max_batch;        /* sequences / images per call, in [1, 16] (the decode MFMA tile's rows;
                           * a prefill of more than 8 runs as row groups of 8)               */
    int max_seq;          /* longest prefill (image + text tokens)                          */
    int max_kv;           /* KV-cache capacity in tokens (decode attention scratch)          */
} pgmi_config;

const char* pgmi_last_error(void);
const char* pgmi_version(void);

/* PaliGemmaForConditionalGeneration.__init__ (modeling_gemma.py:442-453): builds the weight
 * layout; device memory is touched only by the calls below. */
int pgmi_create(int device, const pgmi_config* cfg, pgmi_ctx** out);
int pgmi_destroy(pgmi_ctx* ctx);

/* ---- weights: one bf16 slab in caller-owned device memory, laid out by the library.
 * Tensor names and shapes are the reference state-dict keys; lm_head is
 * tied to embed_tokens (modeling_gemma.py:396-397) and has no slot of its own. */
int64_t pgmi_weights_bytes(const pgmi_ctx* ctx);
int pgmi_weight_count(const pgmi_ctx* ctx);
int pgmi_weight_info(const pgmi_ctx* ctx, int idx, const char** name, int64_t* offset_bytes, int64_t* shape4,
                     int* ndim);
int pgmi_bind_weights(pgmi_ctx* ctx, void* dev_slab);
/* load_state_dict for one tensor (utils.py:30-38 / ablation_study_fixed.py:315-320): copies
 * (and converts to bf16) from host or device memory into the slab. */
int pgmi_load_weight(pgmi_ctx* ctx, const char* name, const void* src, int src_dtype, int src_on_device,
                     void* stream);
/* Native safetensors reader (replaces the safe_open / accelerate
 * shard loop of utils.py:19-44 and ablation_study_fixed.py:304-332): one *.safetensors file is
 * memory-mapped and every tensor whose name is a slab weight is shape-checked, converted to bf16
 * (BF16 copied, F32/F16 rounded to nearest even on the device) and written into the slab.
 * Names that are not slab weights (e.g. a tied lm_head) are counted in *n_skipped.  Synchronises
 * `stream`; call pgmi_prepare again afterwards.  A malformed header or a shape / dtype mismatch
 * is PGMI_E_ARG (ValueError). */
int pgmi_load_safetensors(pgmi_ctx* ctx, const char* path, int* n_loaded, int* n_skipped, void* stream);
/* header inspection, no device needed: tensor count, and entry i's name (NUL-terminated, at most
 * name_cap bytes), dtype (PGMI_DTYPE_*, -1 for other dtypes), shape, data byte range */
int pgmi_safetensors_count(const char* path, int* n);
int pgmi_safetensors_entry(const char* path, int i, char* name, int name_cap, int* dtype, int64_t* shape4, int* ndim,
                           int64_t* begin, int64_t* end);
/* deterministic synthetic weights (benchmarks; oracle/wgen.c recipe) */
int pgmi_fill_synthetic(pgmi_ctx* ctx, const char* name, uint64_t key, float scale, float offset, void* stream);
uint64_t pgmi_synthetic_key(const char* name, uint64_t seed);
/* GemmaRotaryEmbedding.inv_freq (modeling_gemma.py:151), host fp32[head_dim/2]; default is
 * 1/theta^(2i/d) computed as the reference does. */
int pgmi_set_rope_inv_freq(pgmi_ctx* ctx, const float* inv_freq);
/* optional exact cos/sin table (bf16 [max_pos][head_dim/2]) as torch computes it (:178-185) */
int pgmi_set_rope_table(pgmi_ctx* ctx, const uint16_t* cos_tab, const uint16_t* sin_tab, int max_pos);
/* derived device tensors (padded patch-embedding matrix, RoPE table, workspace). Call after
 * the weights are in the slab and before the first forward; synchronises the device. */
int pgmi_prepare(pgmi_ctx* ctx);

/* ---- KV cache (KVCache, modeling_gemma.py:10-36): caller-owned slab
 * [layer][K|V][batch][max_tokens][kv_heads*head_dim] bf16 */
int64_t pgmi_kv_bytes(const pgmi_ctx* ctx, int batch, int max_tokens);

/* ---- forward pieces -------------------------------------------------------------------- */
/* SiglipVisionModel.forward (modeling_siglip.py:236-255) incl. the pixel cast of
 * modeling_gemma.py:570: pixels (B,C,H,W) fp32 or bf16 -> feats (B, N, v_hidden) bf16 */
int pgmi_vision(pgmi_ctx* ctx, const void* pixels, int pixel_dtype, int B, void* feats, void* stream);
/* PaliGemmaMultiModalProjector.forward (modeling_gemma.py:435-438): (rows, v_hidden) -> (rows, proj) */
int pgmi_project(pgmi_ctx* ctx, const void* feats, int rows, void* out, void* stream);
/* nn.Embedding lookup of GemmaModel.embed_tokens (modeling_gemma.py:565) */
int pgmi_embed(pgmi_ctx* ctx, const int64_t* ids, int rows, void* out, void* stream);
/* GemmaForCausalLM.forward (modeling_gemma.py:399-427) over the merged embeddings of
 * _merge_input_ids_with_image_features (modeling_gemma.py:468-537):
 *   ids (device int64 B x L) and image_feats (projected, n_img_rows x hidden, may be NULL) are
 *   merged on the device; if embeds != NULL they are used instead (already-merged embeddings,
 *   e.g. from a monkey-patched merge) and ids/image_feats are ignored.
 *   positions: HOST int64 B x L (rotary positions, modeling_gemma.py:516-535).
 *   KV: keys/values of the L tokens are written at rows kv_start.. of the caller's slab;
 *   attention covers rows [0, kv_start + L) (the reference's zero mask: non-causal).
 *   logits (device fp32): logits_rows == 0 -> (B, L, vocab); 1 -> (B, 1, vocab) last row only;
 *   2 -> (B, 1, vocab) as 1, and no row but the last needs its final hidden state (the generate
 *   loop, inference.py:55-63 takes logits[:, -1, :] only): the last layer writes every row's K/V,
 *   then runs attention, o_proj, the MLP and the final norm for the last row alone (row-wise ops,
 *   so the same values up to accumulation order); pgmi_lm_final_hidden then fails (PGMI_E_STATE). */
int pgmi_lm_forward(pgmi_ctx* ctx, const int64_t* ids, const void* image_feats, int n_img_rows, const void* embeds,
                    int B, int L, const int64_t* positions, void* kv, int kv_batch, int kv_max, int kv_start,
                    float* logits, int logits_rows, void* stream);
/* One KV-cached decode step for B sequences in lock-step (inference.py:56-78 loop body):
 *   ids (device int64 [B]), written at KV row kv_len, rotary position `position`
 *   (= attention_mask.cumsum(-1)[:, -1], modeling_gemma.py:526, i.e. kv_len + 1 after an
 *   inference.py prefill), attention over rows [0, kv_len]; logits (device fp32 [B][vocab]);
 *   next_ids (device int64 [B], may be NULL) = argmax (first max, torch.argmax semantics).
 *   use_graph != 0 replays a captured hipGraph of the whole step.  next_ids == ids feeds the
 *   argmax back in place (tokens are read first, the next ones written last): no staging copy. */
int pgmi_decode(pgmi_ctx* ctx, const int64_t* ids, int B, void* kv, int kv_batch, int kv_max, int kv_len,
                int position, float* logits, int64_t* next_ids, int use_graph, void* stream);
/* n_steps greedy decode steps back to back in one call (one hipGraph launch when use_graph != 0):
 * the generate loop of inference.py:56-78 without sampling, as Engine.generate runs it.  ids (device
 * int64 [B]) holds the input tokens and receives each step's argmax in place (step t + 1 reads step t's);
 * the steps write KV rows kv_len .. kv_len + n_steps - 1 at positions position .. position + n_steps - 1;
 * logits (device fp32 [B][vocab]) holds the last step's; tokens (device int64 [n_steps][B], may be
 * NULL) records every step's argmax.  Each step is pgmi_decode's step, kernel for kernel. */
int pgmi_decode_steps(pgmi_ctx* ctx, int64_t* ids, int B, void* kv, int kv_batch, int kv_max, int kv_len,
                      int position, int n_steps, float* logits, int64_t* tokens, int use_graph, void* stream);
/* ---- ragged batches: every row with its own prompt length ------------------------------------
 * The reference refuses padded batches (modeling_gemma.py:559) and its drop-in modules keep that;
 * these two entries are the engine's own batched driver for prompts of different lengths.  Each row
 * computes what it would compute alone (a batch of one, unpadded).
 *
 * pgmi_lm_forward with per-row lengths: ids is (B, L) right-padded, lens (HOST int32 [B],
 * 1 <= lens[b] <= L) the rows' token counts.  Token j < lens[b] has rotary position positions[b][j]
 * (= j for an inference.py:55-63 prefill) and attends keys [0, kv_start + lens[b]) of its own row,
 * non-causal: the zero mask of modeling_gemma.py:516-535 restricted to the row's real tokens.  Pad
 * slots j >= lens[b] are never looked up (any id is legal there; they enter as zero rows), are never
 * attended by real tokens and never reach a returned value; what is computed for them, and their
 * K/V rows, is unspecified but finite.  logits_rows 1 and 2 return row b's logits at token
 * lens[b] - 1 (2 runs as 1); logits_rows 0 returns all L rows, pad rows unspecified.  embeds must
 * be NULL.  PGMI_E_ARG: a length outside [1, L], B over capacity, null arrays. */
int pgmi_lm_forward_ragged(pgmi_ctx* ctx, const int64_t* ids, const void* image_feats, int n_img_rows,
                           const void* embeds, int B, int L, const int64_t* positions, const int32_t* lens, void* kv,
                           int kv_batch, int kv_max, int kv_start, float* logits, int logits_rows, void* stream);
/* ---- prefix-LM prefill: a prompt attended from everywhere, the tokens after it causally --------
 * pgmi_lm_forward and _ragged are non-causal over the new tokens (the reference's zero mask), which is right for
 * a prompt and wrong for a teacher-forced answer: the row that predicts answer token j + 1 would have attended it.
 * Here row b has a prefix of prefix_lens[b] tokens (HOST int32 [B], 0 <= prefix_lens[b] <= lens[b], or <= L when
 * lens is NULL: the lock-step call).  Token j attends keys [0, kv_start + max(prefix_lens[b], j + 1)) of its own
 * row, never past kv_start + lens[b]: the kv_start cached rows and the prefix from every token, the tokens after
 * the prefix causally.  prefix_lens[b] = 0 is fully causal over the new tokens; prefix_lens[b] = lens[b] for every
 * row launches exactly what pgmi_lm_forward / _ragged launch (bit-identical logits and K/V rows).  Positions are
 * the caller's (to continue with decode steps as the reference counts them, token j >= prefix_lens[b] has position
 * j + 1: the first decode position after an L-token prefill is L + 1).  Embeds are not taken.  logits_rows as
 * pgmi_lm_forward (lens NULL) or _ragged: a row's last token attends all its keys either way.
 * EAGER ONLY: the call runs its launches on the caller's stream; it neither replays, captures nor records a key in
 * the prefill graph cache (pgmi_graph_count is unchanged by it), whatever pgmi_set_prefill_graph says.
 * PGMI_E_ARG: a prefix length outside [0, lens[b]], and everything pgmi_lm_forward(_ragged) refuses. */
int pgmi_lm_forward_prefix(pgmi_ctx* ctx, const int64_t* ids, const void* image_feats, int n_img_rows, int B, int L,
                           const int64_t* positions, const int32_t* lens, const int32_t* prefix_lens, void* kv,
                           int kv_batch, int kv_max, int kv_start, float* logits, int logits_rows, void* stream);
/* n_steps >= 1 decode steps (inference.py:55-78 loop body) for B rows of different lengths: kv_lens
 * and positions are HOST int32 [B].  At step t row b writes K/V at row kv_lens[b] + t, attends keys
 * [0, kv_lens[b] + t] and uses rotary position positions[b] + t (after a ragged prefill
 * positions[b] = lens[b] + 1: attention_mask.cumsum(-1)[:, -1] of modeling_gemma.py:526 for that row
 * alone).  The per-row state lives on the device and is advanced by the step's last kernel, so a call
 * that continues the previous one sets nothing, and graph replay, in-place feedback (next_ids == ids)
 * and the token record work as pgmi_decode / pgmi_decode_steps: logits holds the last step's, next_ids
 * (required when n_steps > 1) every step's argmax in turn, tokens (may be NULL) [n_steps][B].
 * Nothing at or past a row's own length is read.  PGMI_E_ARG: a row with
 * kv_lens[b] + n_steps > kv_max, B over capacity (max_batch, at most 16), null arrays. */
int pgmi_decode_ragged(pgmi_ctx* ctx, const int64_t* ids, int B, void* kv, int kv_batch, int kv_max,
                       const int32_t* kv_lens, const int32_t* positions, int n_steps, float* logits, int64_t* next_ids,
                       int64_t* tokens, int use_graph, void* stream);
/* The same decode step with already-merged input rows instead of token ids: embeds (device bf16
 * [B][hidden]) is the output of a caller's _merge_input_ids_with_image_features for a q_len == 1
 * step (the ablation harness monkey-patches the merge, ablation_study_fixed.py:99-142,335-337,
 * and then calls forward(input_ids=next_token, pixel_values=None, ...) per token, :215-221);
 * the rows are scaled by bf16(sqrt(hidden)) (GemmaModel, modeling_gemma.py:367-368) and run
 * through the same (graph-replayed) step.  The rows are staged into a context buffer first, so
 * the caller's buffer may change between calls. */
int pgmi_decode_embeds(pgmi_ctx* ctx, const void* embeds, int B, void* kv, int kv_batch, int kv_max, int kv_len,
                       int position, float* logits, int64_t* next_ids, int use_graph, void* stream);
/* pgmi_decode_embeds with the step's inputs left on the device (no host read of a merge's outputs):
 * position: the merge's (1, 1) position tensor (attention_mask.cumsum(-1)[:, -1:], modeling_gemma.py:526),
 * dtype PGMI_DTYPE_BF16 / _F32 or 10 = int64, 11 = int32, 12 = float64, rounded to the nearest integer;
 * mask (may be NULL): the merge's additive mask row over the kv_len + 1 keys (modeling_gemma.py:269),
 * bf16 (score + mask rounded to bf16) or fp32 (added in fp32, as torch promotes), row stride
 * mask_b_stride elements.  One sequence (B = 1). */
int pgmi_decode_embeds_dev(pgmi_ctx* ctx, const void* embeds, int B, void* kv, int kv_batch, int kv_max, int kv_len,
                           const void* position, int position_dtype, const void* mask, int mask_dtype,
                           int64_t mask_b_stride, float* logits, int64_t* next_ids, int use_graph, void* stream);
/* Prefill graphs (default on): pgmi_vision and pgmi_lm_forward replay a captured hipGraph when
 * called again with identical pointer and size arguments (the graph is captured on the second
 * such call; a replay reads the same addresses as the eager call would).  0 = always eager. */
int pgmi_set_prefill_graph(pgmi_ctx* ctx, int on);
/* A context keeps two graph caches, the prefill's (pgmi_vision, pgmi_lm_forward*) and the decode steps' (every
 * pgmi_decode* call with use_graph != 0), each keyed by the call's pointer and size arguments and each holding at
 * most PGMI_GRAPH_CACHE_MAX keys: a call whose new key would exceed that drops its whole cache first (and, like any
 * first call with a key, runs eagerly), so callers that pass fresh buffers every time cannot grow it.
 * pgmi_graph_count: the keys a cache holds now (which 0 = prefill, 1 = decode), -1 for a null context. */
#define PGMI_GRAPH_CACHE_MAX 64
int pgmi_graph_count(const pgmi_ctx* ctx, int which);
/* Batched decode (B >= 3, MFMA projections) RMSNorm form: 0 = each input norm computed once per row
 * and read unstaged by the q|k|v / gate|up projections (default), 1 = staged inside each projection,
 * -1 = back to the default.  Same arithmetic either way (bf16 normalised rows);
 * drops captured decode graphs.  A tuning / test switch, no reference counterpart. */
int pgmi_set_decode_staged_norm(pgmi_ctx* ctx, int on);
/* Decode at batch 1-2: lossless 13-bit weight images.  The step's three streaming projections -- gate|up, down
 * and lm_head, 95 % of its bytes -- can read a 13-bit image of their weights instead of the bf16 rows: the
 * sign-and-mantissa byte of every weight plus a 5-bit code of its exponent relative to the tensor's largest
 * (csrc/pack13.h).  The kernels rebuild each bf16 value bit for bit before the same dot products,
 * so every output is identical to the bf16 kernels'; the step streams 13/16 of the bytes.
 *   - Candidate tensors: every layer's gate|up (one tensor) and down, and the tied embedding as lm_head reads it:
 *     2 x layers + 1.  A tensor is packed only if it FITS: no element's exponent field lies in [1, e_hi - 31], e_hi
 *     being the tensor's largest (zeros and denormals, field 0, have a code of their own).  A tensor that does not
 *     fit keeps the bf16 kernel as a whole.
 *   - The images are built on the stream of the first decode step with B <= 2 after a pgmi_prepare (one stream
 *     synchronisation; never inside a caller's capture) and rebuilt after the next pgmi_prepare, which every
 *     weight update must be followed by.  They cost 13/16 of the candidates' bf16 bytes in device memory beside
 *     the bf16 weights, which stay resident for the prefill and the embedding look-up: 3.80 GB at the 3B shapes.
 *     If a kind's buffer cannot be allocated, that kind keeps the bf16 kernels.
 *   - pgmi_set_decode_packed: on = 0 reads the bf16 rows everywhere; on = 1..7 is a mask of the kinds read packed
 *     (1 gate|up, 2 down, 4 lm_head), at B = 1 and B = 2 alike; on < 0 restores the default: the kinds whose
 *     kernel measured faster packed, all three at B = 1 and lm_head alone at B = 2 (two rows double the dot
 *     products per decoded weight: gate|up and down become VALU-limited there).  A change drops the captured decode
 *     graphs of B <= 2 and the prefill graphs (the last-row-only prefill's projections follow the setting); the
 *     batched path (B >= 3) is not touched (its own switch: pgmi_set_decode_packed_batched).  Text hidden 2048 / intermediate 16384 only; other shapes stay raw.
 *   - pgmi_decode_packed_info: info[0] the mask in force at B = 1 ([8]: at B = 2), [1] candidate tensors the
 *     B = 1 step reads packed now, [2] reads raw,
 *     [3] bytes of the packed ones' images, [4] bf16 bytes of the raw ones, [5] 1 if an image allocation failed
 *     since the last pgmi_prepare, [6] 1 if the allocation of the batched (B >= 3) decode's fragment-major images
 *     failed (that path then reads the row-major weights: same results, slower), [7] mask of the kinds scanned
 *     since the last pgmi_prepare.  n >= PGMI_PACKED_INFO_N.
 *   - pgmi_decode_packed_tensor: 1 if the B = 1 step reads the tensor of `kind` (and `layer`; ignored for lm_head)
 *     packed now, 0 if raw. */
#define PGMI_PACKED_INFO_N 9
int pgmi_set_decode_packed(pgmi_ctx* ctx, int on);
int pgmi_decode_packed_info(const pgmi_ctx* ctx, int64_t* info, int n);
int pgmi_decode_packed_tensor(const pgmi_ctx* ctx, int kind, int layer);
/* Batched decode (3..16 rows per step): the same three kinds from a fragment-major 13-bit image.  The MFMA
 * projections of the batched step read, per lane and 128-k block, one 52-byte record instead of four 16-byte bf16
 * fragments, rebuild the fragments bit for bit and feed the same MFMAs in the same order: every output is identical
 * to the bf16 launches', at any batch.  The record is the B <= 2 image's; a segment is one 16-row group x 128-k
 * block (csrc/pack13.h), rows padded to a whole group with zeros.
 *   - pgmi_set_decode_packed_batched: mask 0 (the default) reads the bf16 images everywhere; 1..7 is a mask of the
 *     kinds read packed (1 gate|up, 2 down, 4 lm_head) by every step, stage hook and pgmi_decode_kernel (2, 3, 4)
 *     with B >= 3; anything else is refused.  A change drops the captured decode graphs of B >= 3 and nothing
 *     else; B <= 2 and the prefill (its last-row projections included, at every B) are not touched.
 *   - The images are built like the B <= 2 ones: on the stream of the first B >= 3 step that wants them after a
 *     pgmi_prepare, outside any capture, with one stream synchronisation, one buffer per kind; same candidates, fit
 *     rule and shapes (hidden 2048 / intermediate 16384).  They are held beside the bf16 fragment-major images
 *     and beside any B <= 2 images: up to 3.80 GB more at the 3B shapes with every kind on.  A kind whose buffer
 *     cannot be allocated keeps the bf16 launches ([5]).
 *   - pgmi_decode_packed_batched_info: info[0] the mask, [1] mask of the kinds scanned since the last pgmi_prepare,
 *     [2] candidate tensors the batched step reads packed now, [3] reads raw, [4] bytes of the packed ones' images,
 *     [5] 1 if an image allocation failed since the last pgmi_prepare.  n >= PGMI_PACKED_BATCHED_INFO_N.
 *   - pgmi_decode_packed_batched_tensor: 1 if the batched step reads the tensor of `kind` (and `layer`; ignored for
 *     lm_head) packed now, 0 if raw. */
#define PGMI_PACKED_BATCHED_INFO_N 6
int pgmi_set_decode_packed_batched(pgmi_ctx* ctx, int mask);
int pgmi_decode_packed_batched_info(const pgmi_ctx* ctx, int64_t* info, int n);
int pgmi_decode_packed_batched_tensor(const pgmi_ctx* ctx, int kind, int layer);
/* The 13-bit format on the host (tests; no device): pgmi_pack13_scan gives e_hi and whether n bf16 values fit;
 * pgmi_pack13_bytes the image size of rows x K values (K a multiple of 2048; -1 otherwise); _encode / _decode
 * write the image and rebuild the bf16 values through the functions the kernels use. */
int pgmi_pack13_scan(const uint16_t* w, int64_t n, int* e_hi, int* fits);
int64_t pgmi_pack13_bytes(int64_t rows, int64_t K);
int pgmi_pack13_encode(const uint16_t* w, int64_t rows, int64_t K, int e_hi, uint8_t* image);
int pgmi_pack13_decode(const uint8_t* image, int64_t rows, int64_t K, int e_hi, uint16_t* w);
/* The fragment-major image of the batched step, likewise: ceil(rows / 16) * K / 128 segments of 3,328 bytes (gate|up
 * as one 2 I x K matrix); _decode_mf writes ceil(rows / 16) * 16 rows of K values, the pad rows (+0) included. */
int64_t pgmi_pack13_bytes_mf(int64_t rows, int64_t K);
int pgmi_pack13_encode_mf(const uint16_t* w, int64_t rows, int64_t K, int e_hi, uint8_t* image);
int pgmi_pack13_decode_mf(const uint8_t* image, int64_t rows, int64_t K, int e_hi, uint16_t* w);
/* ---- LoRA adapters (the product of the reference's fine-tuning workflow, SURVEY.md C13: a peft LoraConfig on
 * q_proj / k_proj / v_proj; the PEFT helpers of modeling_gemma.py:458-466,551).  An adapter is merged into the
 * weight slab when it is activated, so the forward kernels do not change and an active adapter costs nothing per
 * token.  The rule (csrc/lora.h), for a target W[N][K] with factors A[r][K], B[N][r] and a scale s in fp32:
 *     acc = 0; for j = 0 .. r-1: acc = acc + (B[n][j] * A[j][k])   (fp32 multiply, then fp32 add: not fused)
 *     W'[n][k] = bf16_rne(fp32(W[n][k]) + acc * s)
 * with W the PRISTINE base every time: one rounding, and switching adapters any number of times cannot drift.
 *   - Up to PGMI_LORA_MAX adapters per context; their factors stay resident on the device as fp32.
 *   - Targets: the 2-D slab weight of any Linear module -- text q/k/v/o_proj and gate/up/down_proj, vision
 *     q/k/v/out_proj, fc1 and fc2, multi_modal_projector.linear.  Embeddings, the 4-D patch convolution, norms,
 *     biases and unknown names are PGMI_E_ARG, as is a factor whose shape does not match its target.
 *   - pgmi_lora_add: a_shape = {r, K}, b_shape = {N, r}; r in [1, 256] is taken from the shapes.  Factors of dtype
 *     PGMI_DTYPE_* in host or device memory (on_device) are widened to fp32 exactly.  Adding to the active adapter,
 *     or a target the adapter already has, is refused (PGMI_E_STATE / PGMI_E_ARG).  Synchronises `stream`.
 *   - pgmi_lora_set(id), id = -1 for the base model: synchronises the device on entry and `stream` on exit, as
 *     pgmi_prepare does; PGMI_E_STATE inside a stream capture.  A target without a valid pristine copy is first
 *     snapshotted (slab -> copy); targets of the outgoing adapter that the incoming one lacks are restored from
 *     their copies; the incoming one's targets are merged copy -> slab.  After pgmi_lora_set(-1) the slab is bit
 *     for bit what it was before the first activation.  Only what depends on a changed tensor is re-derived: the
 *     fragment-major images (B >= 3) when a text-layer projection changed, the 13-bit images of gate|up / down
 *     when a gate_proj or up_proj / a down_proj changed (a q/k/v adapter re-scans nothing); the RoPE tables and
 *     the padded patch matrix never.  Captured graphs are kept where their launches stay valid.
 *   - The pristine copies are forgotten by pgmi_prepare while no adapter is active (the base may have changed)
 *     and by pgmi_bind_weights, which also deactivates; pgmi_prepare while one is active re-derives from the
 *     slab as it is and keeps them.  pgmi_load_weight, pgmi_load_safetensors, pgmi_fill_synthetic and
 *     pgmi_broadcast_weights are PGMI_E_STATE while an adapter is active: deactivate first.
 *   - pgmi_lora_active: the active id, -1 for none (or a null context).  pgmi_lora_info: info[0] the adapter's
 *     targets, [1] bytes of its resident factors, [2] bytes of its targets' pristine copies held now;
 *     n >= PGMI_LORA_INFO_N. */
#define PGMI_LORA_MAX 8
#define PGMI_LORA_INFO_N 3
int pgmi_lora_create(pgmi_ctx* ctx, int* id);
int pgmi_lora_add(pgmi_ctx* ctx, int id, const char* weight_name, const void* A, int a_dtype, const int64_t* a_shape,
                  const void* B, int b_dtype, const int64_t* b_shape, float scaling, int on_device, void* stream);
int pgmi_lora_free(pgmi_ctx* ctx, int id);
int pgmi_lora_set(pgmi_ctx* ctx, int id, void* stream);
int pgmi_lora_active(const pgmi_ctx* ctx);
int pgmi_lora_info(const pgmi_ctx* ctx, int id, int64_t* info, int n);
/* The merge rule on the host (tests; no device): W, out bf16 [N][K], A fp32 [r][K], B fp32 [N][r]. */
int pgmi_lora_merge_host(const uint16_t* W, int64_t N, int64_t K, const float* A, const float* B, int r,
                         float scaling, uint16_t* out);
/* lm_head + .float() of GemmaForCausalLM (modeling_gemma.py:417-418) over final-normed hidden
 * rows: logits (device fp32 [rows][vocab]) = fp32(bf16(normed . E^T)) with the tied embedding E.
 * Together with pgmi_lm_final_hidden this materialises the prefill's all-row logits on demand
 * after a last-row-only pgmi_lm_forward (SURVEY.md sec.7 hard part 3: lazy logits). */
int pgmi_lm_head(pgmi_ctx* ctx, const void* normed, int rows, float* logits, void* stream);
/* Token log-probabilities of the loss of PaliGemmaForConditionalGeneration.forward (modeling_gemma.py:596-603)
 * over final-normed hidden rows, without materialising the logits: with logit[v] = fp32(bf16(normed . E[v])) --
 * bit for bit pgmi_lm_head's whenever that GEMM runs unsplit (always at vocab 257216; a smaller vocabulary's
 * fallback plan can split K at some row counts, and its sums then run in another order) -- lse = logsumexp(logit) and logprob[row] = logit[labels[row]] - lse.  labels: device
 * int64 [rows] (the caller has applied the reference's shift); a row whose label is ignore_index gets 0 (the caller
 * leaves it out of the mean), any other label outside [0, vocab) gets NaN and nothing is read out of bounds.
 * logprob, lse (may be NULL): device fp32 [rows].  The lm_head GEMM's tiles reduce to (max, sum exp) pairs in the
 * context's split-K workspace, rows in chunks that fit it; the order of every sum is fixed (two calls return the
 * same bits).  Stream-ordered, no synchronisation.  PGMI_E_ARG: null pointers, rows < 1, or a forced GEMM
 * configuration (pgmi_tune_gemm) without this epilogue; PGMI_E_STATE before pgmi_prepare. */
int pgmi_lm_logprobs(pgmi_ctx* ctx, const void* normed, int rows, const int64_t* labels, int64_t ignore_index,
                     float* logprob, float* lse, void* stream);
/* The same rule (modeling_gemma.py:596-603) on logits that already exist -- the decode step's device fp32
 * [rows][V]: lse (may be NULL) = logsumexp(logits[row]), logprob[row] = logits[row][ids[row]] - lse, 0 for
 * ids[row] == ignore_index, NaN for any other id outside [0, V).  Stream-ordered, no synchronisation.  Scratch:
 * the context's argmax scratch. */
int pgmi_logprobs(pgmi_ctx* ctx, const float* logits, int rows, int V, const int64_t* ids, int64_t ignore_index,
                  float* logprob, float* lse, void* stream);
/* Copies the final RMSNorm output (GemmaModel.norm, modeling_gemma.py:379) of the B*L rows of the
 * last pgmi_lm_forward (bf16 [rows][hidden], row-major) into `out` (device memory). */
int pgmi_lm_final_hidden(pgmi_ctx* ctx, void* out, int rows, void* stream);

/* ---- replicas: the load-time weight broadcast over RCCL (xGMI).  The
 * reference has no multi-GPU path (accelerate placement only, utils.py:27-38).  One process per
 * GPU: the root calls pgmi_comm_unique_id, ships the PGMI_COMM_ID_BYTES bytes to every rank (any
 * channel), each rank calls pgmi_comm_init, then pgmi_broadcast_weights copies the root's whole
 * weight slab into every replica in one in-place ncclBroadcast; call pgmi_prepare afterwards.
 * A host that already owns an ncclComm_t passes it as `comm` directly. */
#define PGMI_COMM_ID_BYTES 128
int pgmi_comm_unique_id(void* id_out);
int pgmi_comm_init(int device, int nranks, int rank, const void* id, void** comm_out);
int pgmi_comm_destroy(void* comm);
int pgmi_broadcast_weights(pgmi_ctx* ctx, void* comm, int root, void* stream);

/* torch.argmax(logits, -1) over rows of a device fp32 [rows][V] matrix (inference.py:68) */
int pgmi_argmax(pgmi_ctx* ctx, const float* logits, int rows, int V, int64_t* out, void* stream);

/* Stop-token bookkeeping of the batched generate loop (inference.py:51,70-71, per row): rows with
 * finished[b] != 0 get next_ids[b] = pad_id; rows whose next_ids[b] == eos_id are marked finished
 * (their eos is kept, as the reference appends it before breaking).  n_alive (device int32, may be
 * NULL) receives the number of rows still running.  All pointers are device memory. */
int pgmi_eos_update(pgmi_ctx* ctx, int64_t* next_ids, int32_t* finished, int B, int64_t eos_id, int64_t pad_id,
                    int32_t* n_alive, void* stream);

/* Launch one decode kernel of `layer` on the context's decode workspace (benchmarking the
 * dominant kernel in isolation): 1 o_proj+residual, 2 RMSNorm+gate/up+GeGLU, 3 down+residual,
 * 4 final norm + lm_head (+argmax partials; layer ignored). */
int pgmi_decode_kernel(pgmi_ctx* ctx, int which, int layer, int B, void* stream);
/* Test hook: copy `bytes` bytes between the decode workspace pgmi_decode_kernel works on and the caller's device
 * memory `buf` (write != 0: buf -> workspace): which 0 = h (bf16 [max_batch][hidden], kernel 2's input, kernel 1's
 * and 3's in/out), 1 = act (bf16 [max_batch][intermediate], kernel 2's output, 3's input), 2 = kernel 4's logits
 * (fp32 [max_batch][vocab]; stage 5's too).  The buffers pgmi_debug_decode_stage works on besides: 3 = q (bf16
 * [max_batch][heads * head_dim]), 4 = the combined attention output (bf16 [max_batch][hidden]; written at B >= 3
 * only -- at B <= 2 the combine stays in o_proj's registers), 5 = hn, the normed rows the unstaged B >= 3 q|k|v
 * reads (bf16 [max_batch][hidden]), 6 = ssq, o_proj's 16-column partial sums of squares of h (fp32
 * [max_batch][hidden / 16], unstaged B >= 3 only), 7 = the step's next-id buffer (int64 [max_batch]).
 * Stream-ordered.  PGMI_E_ARG: a byte count outside the buffer. */
int pgmi_debug_decode_buffer(pgmi_ctx* ctx, int which, void* buf, int64_t bytes, int write, void* stream);
/* Test hook: copy `bytes` bytes between the flash-decoding partial records and the caller's device memory `buf`
 * (write != 0: buf -> records), as pgmi_debug_decode_buffer does for the other buffers of the decode workspace.
 * Stage 2's attention writes a record per live 64-key chunk and its o_proj combines them: fp32 [max_batch * kv heads]
 * [(max_kv + 63) / 64 chunks][16 * 256 + 32] -- 16 head rows of 256, then 16 chunk maxima and 16 chunk sums.
 * Stream-ordered.  PGMI_E_ARG: a byte count outside the buffer. */
int pgmi_debug_decode_partials(pgmi_ctx* ctx, void* buf, int64_t bytes, int write, void* stream);
/* Test hook: the kernels' in-register cross-lane reductions on their own.  in: device fp32 [rows][64]; one wave
 * reduces each row (four rows per 256-thread workgroup) and writes EVERY lane's result to out, device fp32
 * [rows][64].  op: 0 sum and 1 max over the xor butterfly o = 32, 16, .., 1; 2 first max, the pair (value, index)
 * with a lane's index its lane number, larger value or lower index among equal values, same order; 3 sum over the
 * 16 lanes of a row, o = 1, 2, 4, 8; 4 sum, o = 1, 2, .., 32; 5 sum, o = 16, 32; 6 first max and 7 max over 16
 * lanes, o = 1, 2, 4, 8.  Ops 2 and 6 write the indices, int32 [rows][64], after the rows * 64 values (out holds
 * 2 * rows * 64 words).  PGMI_E_ARG: an unknown op, rows < 1. */
int pgmi_debug_lane_reduce(pgmi_ctx* ctx, int op, const float* in, int rows, float* out, void* stream);
/* Test hook: run ONE stage of the decode step for batch B through the step's own launch code (the functions
 * pgmi_decode's body calls, with the same arguments), at the current pgmi_set_decode_staged_norm /
 * pgmi_set_decode_packed settings, on the decode workspace (pgmi_debug_decode_buffer):
 *   0  the step's entry (layer == 0; other layers: nothing).  B <= 2 with ids: nothing (layer 0's q|k|v folds the
 *      embedding).  B >= 3: embedding x bf16(sqrt(hidden)) -> h, then (unstaged form) layer 0's input norm -> hn.
 *      ids == NULL: h is what the caller wrote into the workspace.             ids / h -> h, hn
 *   1  q|k|v: input norm (or the hn read), projection, RoPE, KV append          h / hn  -> q, KV rows
 *   2  attention partials + combine + o_proj + residual                         q, KV   -> h (B >= 3: ao, ssq)
 *   3  post-attention norm + gate|up + GeGLU                                    h, ssq  -> act
 *   4  down + residual (unstaged B >= 3: + the next layer's input norm -> hn)    act, h  -> h, hn
 *   5  final norm + lm_head + argmax (layer ignored)                            h -> logits (buffer 2), next ids (7)
 * ids: device int64 [B] or NULL (stages 0 and 1 of layer 0 read it).  kv / kv_batch / kv_max: as pgmi_decode.
 * kv_lens / positions: HOST arrays; ragged == 0 reads element 0 of each into the lock-step record, ragged != 0
 * sets one record per row (B entries), as pgmi_decode_ragged.  Every call sets the record(s) it uses, and sets
 * them again after stage 5, whose last kernel advances them.  mask (device, may be NULL; B == 1 only): kv_lens[0]
 * + 1 additive values of mask_dtype bf16 / fp32, the mask of pgmi_decode_embeds_dev.  Eager only: PGMI_E_STATE
 * inside a stream capture.  PGMI_E_ARG: an unknown stage, a layer out of range (stages 1..4), B over capacity,
 * kv_lens[b] + 1 > kv_max, a mask with B != 1. */
int pgmi_debug_decode_stage(pgmi_ctx* ctx, int stage, int layer, int B, const int64_t* ids, void* kv, int kv_batch,
                            int kv_max, const int32_t* kv_lens, const int32_t* positions, int ragged, const void* mask,
                            int mask_dtype, void* stream);
/* Test hook: copy `bytes` bytes between a buffer of the language-model prefill's workspace and the caller's device
 * memory `buf` (write != 0: buf -> workspace), row-major bf16: which 0 = Hs, the hidden state, and 1 = Tn, its norm
 * ([max_batch * max_seq][hidden]: batch row b's slots at rows b * L ..); the scratch one row group (at most 8
 * sequences) holds at a time, [min(max_batch, 8) * max_seq] rows of: 2 = QKV (unrotated q|k|v, written only where the
 * plan has no RoPE epilogue), 3 = Qr (rotated q, heads * head_dim), 4 = AO (attention output, hidden), 5 = ACT
 * (intermediate); 6 = lastrows ([max_batch][hidden], each sequence's last row), 7 = dAO ([max_batch][hidden], the
 * last-row tail's combined attention output).  Stream-ordered.  PGMI_E_ARG: a byte count outside the buffer. */
int pgmi_debug_prefill_buffer(pgmi_ctx* ctx, int which, void* buf, int64_t bytes, int write, void* stream);
/* Test hook: run ONE stage of the language-model prefill for ONE row group (batch rows group * 8 ..) through the
 * prefill's own launch code (the functions pgmi_lm_forward's body calls, with the same arguments), on the prefill
 * workspace (pgmi_debug_prefill_buffer):
 *   0  the entry, for the whole batch (group ignored): merge (ids, image_feats) or embeds x bf16(sqrt(hidden)),
 *      then layer 0's input RMSNorm of every group                              ids / feats / embeds -> Hs, Tn
 *   1  q|k|v with RoPE and the KV append: the fused epilogue, or the GEMM (partial slabs where the plan splits)
 *      and the RoPE kernel, whichever the shape's plan gives                    Tn -> Qr, K/V rows
 *   2  attention over cache rows [0, kv_start + L) (ragged: [0, kv_start + lens[b]))   Qr, K/V -> AO
 *   3  o_proj partial slabs, their sum + residual, the post-attention norm      AO, Hs -> Hs, Tn
 *   4  gate|up + GeGLU                                                          Tn -> ACT
 *   5  down partial slabs, their sum + residual, the next layer's input norm (last layer: the final norm)
 *                                                                               ACT, Hs -> Hs, Tn
 *   6  the logits by logits_rows (layer ignored): 0 every row's (Tn -> logits); 1 each sequence's last row (ragged:
 *      row lens[b] - 1) copied to lastrows, then final norm + lm_head; 2 final norm + lm_head of lastrows as
 *      stage 7 left it                                                          Tn / Hs -> lastrows, logits
 *   7  the last layer's last-row-only tail of logits_rows == 2 (after stage 1 of that layer): the last row's
 *      attention (kv_start + L <= the config's max_kv: the decode step's flash-decoding; else the prefill kernel),
 *      o_proj, MLP and residuals                                                Qr, K/V, Hs -> lastrows
 * Every other argument is pgmi_lm_forward_ragged's, lens == NULL being the lock-step call (pgmi_lm_forward).  Every
 * call copies the host positions to the device and sets the ragged rows' lengths, as those calls do before their
 * launches.  Eager only: it never replays or captures a graph, and returns PGMI_E_STATE inside a stream capture.
 * PGMI_E_ARG: an unknown stage, a layer (stages 1..5, 7) or group (stages 1..7) out of range, stage 7 outside the
 * last layer of a lock-step logits_rows 2 call with L > 1, and everything pgmi_lm_forward(_ragged) refuses.  The
 * final-hidden rows (pgmi_lm_final_hidden) are invalid afterwards. */
int pgmi_debug_prefill_stage(pgmi_ctx* ctx, int stage, int layer, int group, const int64_t* ids,
                             const void* image_feats, int n_img_rows, const void* embeds, int B, int L,
                             const int64_t* positions, const int32_t* lens, void* kv, int kv_batch, int kv_max,
                             int kv_start, float* logits, int logits_rows, void* stream);

/* Image preprocessing on the GPU (processing_paligemma.py:13-49, process_images): PIL-exact
 * BICUBIC resize of one decoded RGB image (uint8 HWC, device memory, H x W) to out_h x out_w,
 * then x/255 (float64 product cast to float32), (x - 0.5)/0.5 and HWC -> CHW, written to
 * `out_chw` (float32 [3][out_h][out_w], device) -- the reference's pixel_values for one image.
 * Uses the context's split-K scratch (stream-ordered with the prefill).  JPEG decode stays on
 * the host. */
int pgmi_preprocess(pgmi_ctx* ctx, const void* src_hwc, int H, int W, int out_h, int out_w, float* out_chw,
                    void* stream);

/* Launch one prefill GEMM of `layer` over `rows` rows of the context's prefill workspace
 * (benchmarking the MFMA path in isolation): 0 = gate|up GEMM + GeGLU epilogue
 * (modeling_gemma.py:134), 1 = down projection (split-K partials, as the prefill runs it). */
int pgmi_prefill_kernel(pgmi_ctx* ctx, int which, int layer, int rows, void* stream);

/* In-situ timing probe of the prefill MLP GEMMs (measurement only): on != 0 makes every following
 * pgmi_lm_forward eager (prefill graphs off) and times each layer's gate|up + GeGLU GEMM and down
 * GEMM kernel (modeling_gemma.py:133-134) with its own start / stop events (hipExtLaunchKernelGGL: the
 * kernel's execution alone); pgmi_prefill_probe_times writes the last probed
 * forward's durations in microseconds: us[i] = layer i's gate|up, us[layers + i] = its down.  on = 0
 * restores the graphs.  Probe with logits_rows 0 or 1: under logits_rows 2 the last layer's MLP runs on the
 * decode GEMVs (no GEMM to time) and pgmi_prefill_probe_times returns PGMI_E_HIP (the unset events). */
int pgmi_prefill_probe(pgmi_ctx* ctx, int on);
int pgmi_prefill_probe_times(pgmi_ctx* ctx, float* us, int n);
/* Tuning hook: force the prefill GEMM tile configuration and split-K factor for subsequent
 * calls (kernels_gemm.hip PGMI_GEMM_CFGS: 11-28 LDS-DMA panel tiles, 30-34 and 38 warp-specialised panel tiles,
 * 36-37 8-phase tiles; an id not in that list is PGMI_E_ARG); a dual (GeGLU) GEMM never splits;
 * cfg < 0 restores the automatic (measured) plan. */
int pgmi_tune_gemm(int cfg, int split);
/* Tuning hook: the same for ONE GEMM shape (M x N x K, dual = the gate|up GeGLU form) while every
 * other shape keeps its plan (in-situ sweeps of a whole forward); cfg < 0 removes the override.
 * Split-K partials that a consumer reduces (out_proj, fc2, down: the residual + norm kernel) are
 * limited to 16 slabs. */
int pgmi_tune_gemm_shape(int M, int N, int K, int dual, int cfg, int split);

/* Test hook: the workgroup -> (row tile, column tile, K slice) order of a panel / 8-phase prefill GEMM
 * launch of n_mt x n_nt tiles x S K slices (tile BM x BN, K deep), as the kernels compute it (the XCD
 * block raster of kernels_gemm.hip xcd_tile); mt/nt/z receive n_mt*n_nt*S entries indexed by the linear
 * workgroup id.  Returns the XCD block code the launch uses (0 = run order); no device needed. */
int pgmi_debug_gemm_tiles(int n_mt, int n_nt, int S, int BM, int BN, int K, int* mt, int* nt, int* z);
/* Test hook: the plan a prefill GEMM of M x N x K (dual = the gate|up GeGLU form) gets -- tile configuration id,
 * tile rows bm and columns bn (dual: per operand), split-K factor -- under the tuning overrides in force; a
 * launch may still lower the split (workspace size, N % 4, empty K ranges).  No device needed. */
int pgmi_debug_gemm_plan(int M, int N, int K, int dual, int* cfg, int* bm, int* bn, int* split);

/* Test hook: what a prefill attention call of head_dim (72 or 256) over B x Lq queries, Lk keys, G query heads per
 * KV head and n_kv KV heads launches (kernels_attn.hip attention_prefill_plan), under the pgmi_tune_attention
 * override in force: kernel 0 = the short one-pass kernel, 1 = the one-pass key-split kernel; compute waves per
 * workgroup (16 query rows each); key ranges and 32-key tiles per range (ranges > 1: the combine kernel follows).
 * kernel 2 with the other three 0: an older kernel family is forced (0, RK or 81 below), which has no such plan.
 * ragged != 0: the call carries per-row key counts; ws_floats: the fp32 scratch it hands over (0: none, no key
 * split).  No device needed. */
int pgmi_debug_attention_plan(int head_dim, int B, int Lq, int Lk, int G, int n_kv, int ragged, int64_t ws_floats,
                              int* kernel, int* waves, int* ranges, int* tiles_per_range);

/* Tuning hook: force the prefill attention kernel (kernels_attn.hip): 7 = one pass with K/V loaded once and
 * scores in registers (head_dim 72, <= 256 keys); 9 = one pass with the keys split over workgroups (online
 * softmax, fp32 partials merged by a combine kernel), 91 / 92 / 94 = the same with 1 / 2 / 4 key ranges;
 * 82 / 81 = the same kernel with 2 / 1 compute waves per workgroup and one key range (head_dim 256); 0 = 16-row
 * kernel with LDS-resident scores; RK = K/V-tiled two-pass kernel with R row groups and K key-split groups per
 * workgroup (41, 42, 21, 22; 44, 24 for head_dim 72); -1 restores the measured choice.  Any other id is
 * PGMI_E_ARG (8, the 16-row kernel with every load up front, was removed).  A forced 7 or 82 that a shape cannot
 * take (the other head_dim, 7 past 256 keys) gets the measured choice for that shape -- it used to fall to the
 * tiled kernel; 0, RK and 81 on a shape or head_dim they do not have still take the tiled kernel 42.  Ragged
 * and prefix-LM calls ignore the override. */
int pgmi_tune_attention(int variant);

/* Nucleus sampling, inference.py:15-24 (_sample_top_p) with inference.py:65's
 * softmax(logits / temperature) fused when temperature > 0 (temperature <= 0: x already holds
 * the probabilities, _sample_top_p's own input).  x: device fp32 [rows][V]; u: device fp32
 * [rows] uniforms in [0, 1) that replace torch.multinomial's internal draw (the token is the
 * first position of the descending order whose cumulative kept mass exceeds u * Z; equal
 * probabilities in index order); out: device int64 [rows]; kept_mass (device fp32 [rows], may
 * be NULL): Z, the renormalisation mass of :21.  Scratch: the context's split-K workspace. */
int pgmi_sample_top_p(pgmi_ctx* ctx, const float* x, int rows, int V, float temperature, float top_p,
                      const float* u, int64_t* out, float* kept_mass, void* stream);

/* Logit processors between a step's logits and the pick (pgmi_argmax / pgmi_sample_top_p): the rule only so far,
 * on host arrays; the device kernels and generate's use of them are left out.  The reference's
 * loop (inference.py:57-71) has none of them; each restates a published rule, and csrc/logits_rule.h states all
 * of them once, in a header that compiles for the host and for the device:
 *   rp   transformers' RepetitionPenaltyLogitsProcessor over prompt and output: x < 0 ? x * rp : x / rp
 *   fp, pp  the OpenAI / vLLM frequency and presence penalties over emitted tokens: x - fp * n_out, x - pp
 *   bias  a dense fp32 [V] row added to every row (transformers' SequenceBiasLogitsProcessor for single tokens;
 *         -inf bans); the caller refuses +inf and NaN entries
 *   suppress_id, min_new_tokens  transformers' MinNewTokensLengthLogitsProcessor: x[suppress_id] = -inf while
 *         emitted[row] < min_new_tokens (suppress_id < 0 or min_new_tokens <= 0: off)
 *   top_k  transformers' TopKLogitsWarper, by value (ties at the k-th value all stay); 0 or >= V: off
 *   min_p_delta  transformers' MinPLogitsWarper decided in logit space: keep y >= max(y) + delta with
 *         delta = fp32(T * ln(min_p)) <= 0 from the host; -inf: off
 * in that order; the two thresholds are one, max(kth, max + delta).  A row the first four leave without a finite
 * maximum comes back as the raw x (pgmi_argmax has no index for such a row).  A neutral parameter's step is
 * skipped, so all-neutral parameters copy x bit for bit. */
typedef struct pgmi_logits_params {
    float rp, pp, fp;
    int top_k;
    float min_p_delta;
    int suppress_id;
    int min_new_tokens;
} pgmi_logits_params;
/* y (fp32 [rows][V], y == x allowed) = the rule applied to x, all host arrays; the k-th value by a sort.  No
 * context, no GPU.  history: uint32 [rows][V], word v = (v occurs in the row's prompt) << 31 | times the row has
 * emitted v; NULL allowed when rp == 1 and pp == fp == 0.  bias (fp32 [V]) may be NULL; emitted (int32 [rows],
 * tokens each row has emitted so far) may be NULL when the suppress is off.  PGMI_E_ARG: rp <= 0 or a non-finite
 * penalty, top_k < 0, min_p_delta > 0 or NaN, a penalty without a history, a suppress without emitted or with
 * suppress_id >= V, rows or V <= 0. */
int pgmi_logits_process_host(const float* x, int rows, int V, const uint32_t* history, const float* bias,
                             const pgmi_logits_params* params, const int32_t* emitted, float* y);

/* ---- beam search: the rule, on the host only so far (csrc/beam_rule.h, DESIGN.md sec.1 (m): the device step and the
 * KV gather are left out of the tree): transformers' _beam_search with do_sample=False, one stop
 * token and early_stopping in {False, True}.  G groups (prompts) of K beams, G * K <= max_batch <= 16; C = 2K
 * candidates per step; steps t = 0 .. n_tokens - 1, t = 0 picking from the prefill's logits (rows_in = 1, one row per
 * group), every later one from the decode step's (rows_in = K).  A candidate of input row r scores
 * s = fp32(fp32(x - lse_r) + run_r); the group keeps the first C by (s descending, row ascending, then x descending,
 * token ascending within a row).  Candidates that are not eos carry on as the K running beams; eos candidates among
 * the first K (on the last step: every one) contest the group's pool of K finished hypotheses with s / den[t + 1],
 * den[n] = fp32(double(n) ** length_penalty) from the host.  A group is frozen (its pool final) once its best running
 * score can no longer beat the pool's worst, or with early_stopping once the pool is full.
 *
 * The state is one caller-allocated blob of pgmi_beam_state_bytes() bytes, 16-byte aligned: a header, den, the running
 * scores, flags, pool, the parent / token history of every step, and room for a device step's scratch.
 * pgmi_beam_state_layout gives the offsets in 4-byte words: out[0..13] = den, run, heur, frozen, pool_score,
 * pool_valid, pool_step, pool_parent, pool_token, hist_parent, hist_token, words of the state proper (what a final
 * read copies), words in all, slices per row.  Sequences are rebuilt on the host: a pool slot (step, parent row,
 * token) is walked back through hist_token[u][row], hist_parent[u][row], u = step - 1 .. 0.
 * pgmi_beam_state_bytes is -1, and the others PGMI_E_ARG, unless 1 <= K <= 16, G * K <= 16, n_tokens >= 1 and
 * 2K <= V <= 1.5M; eos is -1 (none) or in [0, V). */
int64_t pgmi_beam_state_bytes(int G, int K, int n_tokens, int V);
int pgmi_beam_state_layout(int G, int K, int n_tokens, int V, int64_t* out, int n);
/* The rule on the host: no context, no GPU.  `state` is host memory of at least the state proper.  lse_in (fp32
 * [G * rows_in]) may be NULL: the host then takes each row's log-sum-exp in fp64 itself; lse_out, n_open may be NULL.
 * next_ids int64 [G * K], parent int32 [G * K] (batch rows g * K + beam; in range whatever the logits hold). */
int pgmi_beam_reset_host(void* state, int G, int K, int n_tokens, int V, int eos, int early_stopping, const float* den);
int pgmi_beam_step_host(void* state, const float* logits, int rows_in, int t, const float* lse_in, int64_t* next_ids,
                        int32_t* parent, int32_t* n_open, float* lse_out);
/* ---- single-op entry points (kernel-level parity tests) ---------------------------------- */
/* out = epilogue(A[M,K] . W[N,K]^T): epi 0 store, 1 +bias, 2 +bias,gelu, 3 +bias,+res, 4 +res,
 * 6 fp32 out (out is float*), 7 GeGLU with up rows at W + N*K */
int pgmi_op_gemm(pgmi_ctx* ctx, const void* A, const void* W, int M, int N, int K, int epi, const void* bias,
                 const void* res, void* out, void* stream);
/* pgmi_lm_logprobs (the loss of modeling_gemma.py:596-603) on a caller's W[V][K] (bf16, row-major) in place of the
 * tied embedding: normed is [rows][K].  K a multiple of 8.  The logits it reduces are pgmi_op_gemm(epi 6)'s on the
 * same operands, bit for bit, whenever that GEMM runs unsplit. */
int pgmi_op_lm_logprobs(pgmi_ctx* ctx, const void* normed, const void* W, int rows, int V, int K,
                        const int64_t* labels, int64_t ignore_index, float* logprob, float* lse, void* stream);
/* pgmi_op_gemm with explicit row strides (elements, multiples of 8, >= K) of A and W: the prefill GEMMs'
 * sensitivity to the operands' row pitch (tools/probes/stride_probe.py). */
int pgmi_op_gemm_strided(pgmi_ctx* ctx, const void* A, int lda, const void* W, int ldw, int M, int N, int K, int epi,
                         const void* bias, const void* res, void* out, void* stream);
int pgmi_op_rmsnorm(pgmi_ctx* ctx, const void* x, const void* w, int rows, int D, float eps, void* out,
                    void* stream);
int pgmi_op_layernorm(pgmi_ctx* ctx, const void* x, const void* w, const void* b, int rows, int D, float eps,
                      void* out, void* stream);
/* out = bf16(a + b) elementwise over n bf16 values (n a multiple of 8): the residual adds of the per-layer
 * module forwards (SiglipEncoderLayer.forward modeling_siglip.py:189,202; GemmaDecoderLayer :327,336) */
int pgmi_op_add(pgmi_ctx* ctx, const void* a, const void* b, int64_t n, void* out, void* stream);
/* SiglipVisionEmbeddings.forward (modeling_siglip.py:62-79) on given parameters: pixels (B, C, H, H)
 * bf16 or fp32 (pixel_dtype), conv weight [D][C][P][P] + bias [D], position embedding [(H/P)^2][D]
 * -> out (B, (H/P)^2, D) bf16 = bf16(bf16(conv + bias) + pos); uses the context's scratch */
int pgmi_op_patch_embed(pgmi_ctx* ctx, const void* pixels, int pixel_dtype, int B, int C, int H, int P,
                        const void* conv_w, const void* conv_b, const void* pos, int D, void* out, void* stream);
/* attention over q (B, Lq, H, hd), k/v (B, Lk, Hkv, hd) -> o (B, Lq, H, hd), all contiguous bf16;
 * s = bf16(bf16(q.k) * scale) */
int pgmi_op_attention(pgmi_ctx* ctx, const void* q, const void* k, const void* v, void* o, int B, int Lq, int Lk,
                      int H, int Hkv, int head_dim, float scale, void* stream);
/* Reference-order attention of the module forwards (SiglipAttention.forward modeling_siglip.py:116-131,
 * GemmaAttention.forward modeling_gemma.py:262-277), returning the probability matrix the reference
 * returns as its second output:
 *   s = bf16(q.k); s = bf16(s * scale) (scale_div 0) or bf16(s / scale) (scale_div 1, Gemma's
 *   "/ math.sqrt(head_dim)"); + mask (additive, optional: bf16 -> bf16(s + m), fp32 -> s + m in fp32,
 *   as torch promotes); p = bf16(softmax_fp32(s)); o = bf16(p.v).  q/o (B, Lq, H, hd); k/v
 *   (B, Lk, Hkv, hd) for kv_layout 0 or (B, Hkv, Lk, hd) for kv_layout 1 (the KVCache layout);
 *   query head h reads KV head h / (H / Hkv) (repeat_kv, :136-141).  mask element (b, h, i, j) at
 *   b*m_b_stride + h*m_h_stride + i*m_q_stride + j (a stride of 0 broadcasts).  probs (B, H, Lq, Lk)
 *   bf16, may be NULL.  hd <= 256. */
int pgmi_op_attention_ex(pgmi_ctx* ctx, const void* q, const void* k, const void* v, void* o, int B, int Lq, int Lk,
                         int H, int Hkv, int head_dim, int kv_layout, float scale, int scale_div, const void* mask,
                         int mask_dtype, int64_t m_b_stride, int64_t m_h_stride, int64_t m_q_stride, void* probs,
                         void* stream);
/* The prefill attention of pgmi_lm_forward_prefix on raw bf16 buffers, through the launcher the prefill uses (not
 * the reference-order kernel of pgmi_op_attention_ex): q/o (B, Lq, H, hd), k/v rows of Lk keys per batch row in
 * kv_layout 0 (B, Lk, Hkv, hd) or 1 (B, Hkv, Lk, hd), hd = 256, B <= 16.  Query j of row b attends keys
 * [0, min(klen[b], kv_start + max(prefix_lens[b], j + 1))); klen (HOST int32 [B], kv_start < klen[b] <= kv_start +
 * Lq <= Lk; NULL: kv_start + Lq for every row) and prefix_lens (HOST int32 [B], 0 <= prefix_lens[b] <= klen[b] -
 * kv_start).  Keys at or past a row's klen[b] are never read.  s = bf16(bf16(q.k) * scale). */
int pgmi_op_attention_prefix(pgmi_ctx* ctx, const void* q, const void* k, const void* v, void* o, int B, int Lq,
                             int Lk, int H, int Hkv, int head_dim, int kv_layout, float scale, int kv_start,
                             const int32_t* klen, const int32_t* prefix_lens, void* stream);
/* The key ranges (>= 1) the kernel of pgmi_op_attention_prefix splits the kv_start + Lq keys of such a call into on
 * this context (more than one: partials in the context's scratch, merged by a second kernel); negative: an error. */
int pgmi_op_attention_prefix_splits(pgmi_ctx* ctx, int B, int Lq, int H, int Hkv, int kv_start);
/* apply_rotary_pos_emb for one projection (modeling_gemma.py:187-199) with the caller's cos/sin rows
 * (GemmaRotaryEmbedding.forward's output, :155-185): x (rows, heads*hd) -> out = bf16(bf16(x*cos) +
 * bf16(rotate_half(x)*sin)), cos/sin bf16 (rows, hd). */
int pgmi_op_rope(pgmi_ctx* ctx, const void* x, const void* cos_rows, const void* sin_rows, int64_t rows, int heads,
                 int head_dim, void* out, void* stream);
/* out = bf16(x * a) over n bf16 values (n a multiple of 8): GemmaModel's normalizer (modeling_gemma.py:367-368) */
int pgmi_op_scale(pgmi_ctx* ctx, const void* x, float a, int64_t n, void* out, void* stream);
/* the LoRA merge kernel on caller tensors (device; 16-B aligned): W, out bf16 [N][K] (not overlapping), A fp32
 * [r][K], B fp32 [N][r]; K a multiple of 8, r in [1, 256].  Bit for bit pgmi_lora_merge_host. */
int pgmi_op_lora_merge(pgmi_ctx* ctx, const void* W, int N, int K, const void* A, const void* B, int r,
                       float scaling, void* out, void* stream);
/* decode GEMV family on one layer's weights (tests): y[b][n] += W x (residual form); B in [1, 16], K 2048 or 16384 */
int pgmi_op_gemv_res(pgmi_ctx* ctx, const void* x, const void* W, int B, int N, int K, void* h_inout,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PGMI_H */
