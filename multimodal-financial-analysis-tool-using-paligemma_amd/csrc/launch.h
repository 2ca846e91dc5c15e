// launch.h -- host-side launchers for the libpgmi kernels (internal, not the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pgmi {

// ---------------------------------------------------------------- GEMM (prefill)
enum Epi : int {
    EPI_STORE = 0,      // out = bf16(acc)
    EPI_BIAS = 1,       // out = bf16(acc + bias)
    EPI_BIAS_GELU = 2,  // out = bf16(gelu(bf16(acc + bias)))
    EPI_BIAS_RES = 3,   // out = bf16(bf16(acc + bias) + res)
    EPI_RES = 4,        // out = bf16(bf16(acc) + res)
    EPI_BIAS_POS = 5,   // out = bf16(bf16(acc + bias) + pos[m % npos])
    EPI_F32 = 6,        // out_f32 = float(bf16(acc))
    EPI_GEGLU = 7,      // out = bf16(bf16(gelu(bf16(acc_gate))) * bf16(acc_up))  (dual B)
    EPI_ROPE = 8,       // Gemma q|k|v rows: RoPE on q and k, q -> q_out, k / v appended to the KV cache
                        // (modeling_gemma.py:197-198,259); gemm_qkv_rope only
    EPI_LSE = 9,        // no output matrix: per (row, column tile) the pair (max, sum exp(x - max)) of x = bf16(acc),
                        // and x at the row's label column (modeling_gemma.py:596-603); gemm_lse only
};

struct EpiArgs {
    const uint16_t* bias = nullptr;
    const uint16_t* res = nullptr;  // [M][ldr]
    int ldr = 0;
    const uint16_t* pos = nullptr;  // [npos][N]
    int npos = 0;
    uint16_t* out = nullptr;        // [M][ldo]
    int ldo = 0;
    float* out_f32 = nullptr;       // [M][ldo]
    // EPI_ROPE: rows m = b * L + l at rotary position rpos[m]; heads [0, nh) are q (-> q_out
    // [M][nh*256]), nh .. nh+nkv-1 are k, the rest v (-> kc / vc at token kv_start + l)
    const int64_t* rpos = nullptr;
    const uint16_t* cosT = nullptr;
    const uint16_t* sinT = nullptr;
    int max_pos = 0;
    uint16_t* q_out = nullptr;
    uint16_t* kc = nullptr;
    uint16_t* vc = nullptr;
    long kv_b_stride = 0;
    int kv_start = 0;
    int L = 1;
    int nh = 0;
    int nkv = 0;
    // EPI_LSE: row m's label column lse_labels[m] (any value; one outside [0, N) selects nothing), the pair of
    // column tile nt -> lse_part[m * lse_nt + nt], the label's logit -> lse_lab[m]
    const int64_t* lse_labels = nullptr;
    float2* lse_part = nullptr;
    float* lse_lab = nullptr;
    int lse_nt = 0;
};

// C[M,N] = A[M,K] (row-major, lda) x W[N,K]^T (row-major, ldw).  For EPI_GEGLU the
// "up" weight rows are W + up_offset_rows*ldw.  `ws` is fp32 scratch for split-K.
// Returns the split-K factor used.  With defer = true and a split > 1 only the fp32 partial
// slabs ws[split][M][N] are written and the epilogue is left to the consumer kernel
// (splitk_res_norm / rope_kv_append); otherwise the epilogue is applied and 1 is returned.
// q|k|v projection with the RoPE / KV-append epilogue (EPI_ROPE) when the measured plan for the
// shape allows it (two 16-column tiles per wave, no split-K); false: nothing launched, the caller
// runs gemm(EPI_STORE) + rope_kv_append
bool gemm_qkv_rope(hipStream_t s, const uint16_t* A, int lda, const uint16_t* W, int ldw, int M, int N, int K,
                   const EpiArgs& ea);
int gemm(hipStream_t s, const uint16_t* A, int lda, const uint16_t* W, int ldw, int M, int N, int K,
         Epi epi, const EpiArgs& ea, float* ws, size_t ws_bytes, int up_offset_rows = 0, bool defer = false);
size_t gemm_ws_bytes(int M, int N, int K);
// The lm_head GEMM without its output (EPI_LSE): the plan gemm() takes for the shape, never split, so each logit is
// bit for bit the one gemm(EPI_F32) writes.  part: [M][gemm_lse_tiles(M, N, K)] pairs, lab: [M].  gemm_lse_tiles
// returns 0 when the shape's (or the forced) tile configuration has no EPI_LSE instance; gemm_lse then launches
// nothing and returns false.  lse_combine merges each row's pairs in ascending tile order (fp64) into lse[row]
// (may be null) and logprob[row] = lab[row] - lse[row]: 0 for labels[row] == ignore_index, NaN for any other
// label outside [0, N).
int gemm_lse_tiles(int M, int N, int K);
bool gemm_lse(hipStream_t s, const uint16_t* A, int lda, const uint16_t* W, int ldw, int M, int N, int K,
              const int64_t* labels, float2* part, float* lab);
void lse_combine(hipStream_t s, const float2* part, int n_nt, const float* lab, const int64_t* labels, int rows, int N,
                 int64_t ignore_index, float* logprob, float* lse);
void gemm_force_plan(int cfg, int split);  // cfg < 0: automatic
int gemm_force_shape(int M, int N, int K, int dual, int cfg, int split);  // cfg < 0: remove the override
// probe: the next GEMM kernel launched takes these events as its own start / stop (hipExtLaunchKernelGGL)
void gemm_probe_events(hipEvent_t start, hipEvent_t stop);
// host replica of the panel / 8-phase GEMMs' workgroup -> tile order (CPU test); returns the XCD block code
int gemm_tile_order(int n_mt, int n_nt, int S, int BM, int BN, int K, int* mt, int* nt, int* z);
bool gemm_cfg_valid(int cfg);              // a tile configuration of kernels_gemm.hip's list (PGMI_GEMM_CFGS)
// the plan a GEMM of this shape runs (tile configuration id, tile rows / columns, split-K factor); no device needed
void gemm_plan(int M, int N, int K, int dual, int* cfg, int* bm, int* bn, int* split);

// ---------------------------------------------------------------- decode GEMV
// A launcher that cannot launch (a kernel attribute the runtime refuses, a batch no kernel form covers) records
// the error here and launches nothing; the engine's launch check takes it with the launch errors
// (hipSuccess: none since the last take).
void launch_error_set(hipError_t e, const char* what);
hipError_t launch_error_take(const char** what);
struct StepState {  // device-resident decode step (read by kernels -> graph-replayable)
    int kv_len;     // index the new token's K/V is written at (= KVCache.num_items())
    int position;   // rotary position (= attention_mask.cumsum(-1)[:, -1], modeling_gemma.py:526)
};
// The record is an array: batch row b reads st[b * st_stride].  st_stride = 0 is the lock-step step (one
// record shared by every row), st_stride = 1 the ragged step (pgmi_decode_ragged: a record per row, each
// row with its own KV write row, attended key count and rotary position).  The step's last kernel
// advances records [0, adv_n): 1 on the lock-step path, B on the ragged one.

// decode layer 0: the embedding lookup folded into the q|k|v GEMV (h_out receives the scaled row)
struct EmbedFold {
    const int64_t* ids;
    const uint16_t* E;
    float normalizer;
    int64_t pad_id;
    uint16_t* h_out;
};
bool gemv_qkv_folds_embed(int B);  // batches the fold covers (the register-input GEMV, B <= 2)
// fused input RMSNorm + q/k/v projection + RoPE + KV-cache append (K = 2048)
void gemv_qkv(hipStream_t s, int B, int nh, int nkv, const uint16_t* h, const uint16_t* norm_w, float eps,
              const uint16_t* Wqkv, const uint16_t* cosT, const uint16_t* sinT, int max_pos, const StepState* st,
              uint16_t* q_out, uint16_t* kc, uint16_t* vc, long kv_b_stride, float* ws = nullptr,
              const EmbedFold* emb = nullptr, const uint16_t* Wf = nullptr,  // Wf: as gemv_geglu's
              int st_stride = 0);
// The 13-bit image of a weight matrix (pack13.h) for the streaming GEMVs at B <= 2 (gate|up, down at K = 16384,
// lm_head): img null = read the bf16 rows; base2 = pk_base2(e_hi).  Same outputs, bit for bit, either way.
// At B >= gemv_mf_min_batch() the same arguments take the image's fragment-major form (PK_FORM_FRAG) for the MFMA
// forms.  A launcher is handed the image of the form its batch reads (pk_use), never both.
struct PkW {
    const uint8_t* img = nullptr;
    unsigned base2 = 0;
};
// pass one / two of the image build (kernels_pack.hip): stat[0] = largest exponent field, stat[1] = smallest
// one >= 1 (caller presets 0 / 0xFFFFFFFF); form: a PkForm (pack13.h) -- row-major segments for the streaming GEMVs
// (B <= 2), fragment-major ones for the MFMA GEMVs; out: pk_image_bytes(form, rows, K) bytes, K a multiple of 2048
void pk_scan(hipStream_t s, const uint16_t* W, long numel, unsigned* stat);
void pk_pack(hipStream_t s, int form, const uint16_t* W, long rows, int K, int e_hi, uint8_t* out);
// LoRA (kernels_lora.hip, the rule of lora.h): out[N][K] = bf16(W + (B . A) * scaling) from the pristine W (bf16),
// A[r][K] and B[N][r] in fp32 (all 16-B aligned, K a multiple of 8, r in [1, 256]); out does not overlap W.  lora_widen:
// n factor values of dtype PGMI_DTYPE_* on the device to fp32.
void lora_merge(hipStream_t s, const uint16_t* W, int N, int K, const float* A, const float* B, int r, float scaling,
                uint16_t* out);
void lora_widen(hipStream_t s, const void* src, int dtype, long n, float* dst);
// ws: fp32 scratch (>= 4 x B x N floats) for the MFMA path's K split of K = 16384 (B >= 3)
void gemv_res(hipStream_t s, int B, int K, const uint16_t* x, const uint16_t* W, int N, uint16_t* h_inout,
              float* ws, PkW pk = {});
// gemv_res, then hn = RMSNorm(h) with norm_w (nullptr: none); on the batched MFMA path the norm is
// fused into the K-split combine (one workgroup per row)
void gemv_res_norm(hipStream_t s, int B, int K, const uint16_t* x, const uint16_t* W, int N, uint16_t* h_inout,
                   float* ws, const uint16_t* norm_w, float eps, uint16_t* hn, const uint16_t* Wf = nullptr,
                   PkW pk = {});
// the fragment-major image of a [rows][K] matrix for the batched decode GEMVs (rows % 16 == 0, K % 32 == 0)
// (qkv: in the batched q|k|v GEMV's row order)
void mf_swizzle(hipStream_t s, const uint16_t* W, int rows, int K, uint16_t* out, bool qkv = false);
// hn[b] = RMSNorm(x[b]) for nb rows of K (one workgroup per row)
void rows_norm(hipStream_t s, const uint16_t* x, const uint16_t* w, float eps, int nb, int K, uint16_t* out);
// o_proj + residual whose input is the combine of the decode-attention partials (MQA:
// n_kv = 1, G heads of 256); o_out (optional) receives the combined bf16 attention output.
// ssq (batched MFMA form only, else ignored): each row's 16-column partial sums of squares of the
// new h, [B][N / 16] -- the next RMSNorm's, read by gemv_geglu
void gemv_o_attn(hipStream_t s, int B, int G, const float* part, int max_chunks, const StepState* st,
                 const uint16_t* Wo, int N, uint16_t* h_inout, uint16_t* o_out, float* ssq = nullptr,
                 const uint16_t* Wf = nullptr, int st_stride = 0);
// fused RMSNorm + gate|up + GeGLU; ssq (B >= gemv_mf_min_batch() only): h's RMSNorm from the
// partials gemv_o_attn wrote instead of the row pass; Wf (idem): the gate|up weights' fragment-major
// image (mf_swizzle: the gate rows', then the up rows'), read instead of Wgu
void gemv_geglu(hipStream_t s, int B, const uint16_t* h, const uint16_t* norm_w, float eps,
                const uint16_t* Wgu, int I, uint16_t* act, float* ssq = nullptr, const uint16_t* Wf = nullptr,
                PkW pk = {});
int gemv_logits_blocks();
int gemv_mf_min_batch();  // smallest batch on the MFMA decode projections
// done/next/adv (decode, may be null): fold the argmax into the launch's last workgroup and
// advance the step state there; returns true when it did (no argmax_finish needed)
bool gemv_logits(hipStream_t s, int B, const uint16_t* h, const uint16_t* norm_w, float eps,
                 const uint16_t* E, int V, float* logits, float* pmax, int* pidx, int* nparts,
                 unsigned* done = nullptr, int64_t* next = nullptr, StepState* adv = nullptr,
                 int64_t* hist = nullptr, int adv_n = 1, PkW pk = {});
// adv (may be null): the decode step state, advanced by one step (the step's last kernel); hist (may be
// null): a second destination of the argmax (a multi-step graph's per-step token record)
void argmax_finish(hipStream_t s, int B, const float* pmax, const int* pidx, int nparts, int64_t* out,
                   StepState* adv = nullptr, int64_t* hist = nullptr, int adv_n = 1);
int argmax_scratch_parts();
void argmax_rows(hipStream_t s, const float* x, int rows, int V, float* pmax, int* pidx, int64_t* out);
// common.h's in-register reductions on rows of 64 fp32 values, one wave per row and four rows per workgroup; every
// lane's result is written: out[row][lane] (ops kLaneFirstMax / kLaneRow16FirstMax: the indices, int32
// [rows][64], follow the rows * 64 values; a lane's starting index is its lane number)
enum LaneReduceOp {
    kLaneSum = 0,            // wave_sum: o = 32, 16, .., 1
    kLaneMax = 1,            // wave_max
    kLaneFirstMax = 2,       // wave_first_max
    kLaneRow16Sum = 3,       // row16_sum_asc: o = 1, 2, 4, 8
    kLaneSumAsc = 4,         // o = 1, 2, .., 32
    kLaneQuarterSum = 5,     // o = 16, 32
    kLaneRow16FirstMax = 6,  // row16_first_max_asc
    kLaneRow16Max = 7,       // row16_max_asc
    kLaneReduceOps = 8
};
void lane_reduce_rows(hipStream_t s, int op, const float* in, int rows, float* out);
// lse[row] (may be null) = logsumexp(x[row]) and logprob[row] = x[row][ids[row]] - lse[row] over fp32 rows
// [rows][V] (0 for ids[row] == ignore_index, NaN for any other id outside [0, V)); pm / ps: scratch of
// argmax_scratch_parts() floats each
void logprob_rows(hipStream_t s, const float* x, int rows, int V, const int64_t* ids, int64_t ignore_index, float* pm,
                  float* ps, float* logprob, float* lse);
void eos_update(hipStream_t s, int64_t* next, int* finished, int B, int64_t eos, int64_t pad, int* n_alive);

// ---------------------------------------------------------------- attention
struct AttnArgs {
    const uint16_t* q; long q_b_stride; int q_row_stride; int q_head_stride;
    const uint16_t* k; long k_b_stride; int k_row_stride; int k_head_stride;
    const uint16_t* v; long v_b_stride; int v_row_stride; int v_head_stride;
    uint16_t* o; long o_b_stride; int o_row_stride; int o_head_stride;
    int Lq;        // query positions per batch element
    int Lk;        // keys
    int G;         // query heads per kv head
    int n_kv;      // kv heads
    int B;
    float scale;   // s = bf16(bf16(q.k) * scale)
    float* ws;     // prefill: fp32 scratch for key-split partials (nullptr: no key split)
    long ws_floats;
    // decode: additive attention mask (modeling_gemma.py:269), fp32, key j of batch row b at
    // mask[b * mask_b_stride + j * mask_k_stride]; mask_round: the sum is rounded to bf16 (a bf16
    // mask) or kept in fp32 (an fp32 mask, as torch promotes).  No mask: a zero word with stride 0
    const float* mask;
    long mask_b_stride;
    int mask_k_stride;
    int mask_round;
    // ragged prefill: batch row b attends keys [0, klen[b]) (a device array, klen[b] <= Lk); nullptr: Lk
    // keys for every row.  Honoured by the one-pass key-split kernel, which ragged prefills always take
    const int* klen;
};
void attention_prefill(hipStream_t s, int head_dim, const AttnArgs& a);
// What a prefill attention call of this shape launches, under the tuning override in force: kernel 0 = the short
// one-pass kernel (head dim 72, <= 256 keys), 1 = the one-pass key-split kernel; nw = compute waves per workgroup
// (16 query rows each); ns key ranges of tps 32-key tiles (ns > 1: the combine kernel follows).  kernel 2 (the
// other fields 0): a forced variant of the older families, which only the tuning hook reaches.  ragged: the call
// sets klen; ws_floats: the fp32 scratch it hands over (0: none).  A pure host function: no device needed.
struct AttnPlan {
    int kernel, nw, ns, tps;
};
AttnPlan attention_prefill_plan(int head_dim, int B, int Lq, int Lk, int G, int n_kv, bool ragged, long ws_floats);
// prefix-LM prefill (head dim 256, klen set): query position j of batch row b attends keys [0, min(klen[b],
// kv_start + max(pfx[b], j + 1))) -- the kv_start cached rows and the row's prefix (pfx, a device array indexed like
// klen) from everywhere, the rest causally.  The argument of the one-pass key-split kernel's prefix instances alone:
// every other attention kernel takes AttnArgs as it was
struct AttnPrefixArgs : AttnArgs {
    const int* pfx;
    int kv_start;
};
void attention_prefill_prefix(hipStream_t s, const AttnPrefixArgs& a);
// the key ranges the one-pass key-split kernel takes for a ragged or prefix call of these arguments (head dim 256)
int attention_prefill_splits(const AttnArgs& a);
// decode: Lq == 1, rows = the G heads; keys split over chunks; kv length from StepState (+1)
// flash-decoding over 64-key chunks (partials only; the combine is gemv_o_attn's prologue);
// launch_keys = upper bound on kv_len+1 this call
void attention_decode(hipStream_t s, const AttnArgs& a, const StepState* st, int launch_keys, float* part,
                      int max_chunks, int st_stride = 0);
constexpr int kAttnChunk = 64;
constexpr int kAttnPartStride = 16 * 256 + 32;  // floats per (b, kv head, chunk) record
size_t attention_decode_part_floats(int B, int n_kv, int max_chunks);
void attention_force_variant(int v);  // tuning hook (kernels_attn.hip); -1 = measured choice
// the process-wide count of tuning calls (pgmi_tune_gemm, pgmi_tune_gemm_shape, pgmi_tune_attention), an element
// of every prefill graph key (engine_graph.h): bump = 1 counts one more call; returns the count
__attribute__((visibility("hidden"))) long tune_epoch(int bump = 0);

// ---------------------------------------------------------------- per-module entry points (kernels_modules.hip)
// reference-order attention with the probability matrix and an additive mask (module forwards)
struct ModAttnArgs {
    const uint16_t* q;           // (B, Lq, H, hd)
    const uint16_t* k;           // KV head hk of batch b, key j: k + b*kv_b_stride + hk*kv_h_stride + j*kv_row_stride
    const uint16_t* v;
    long kv_b_stride, kv_h_stride, kv_row_stride;
    uint16_t* o;                 // (B, Lq, H, hd)
    uint16_t* probs;             // (B, H, Lq, Lk) bf16 or nullptr
    const void* mask;            // additive, element (b, h, i, j) at b*m_b_stride + h*m_h_stride + i*m_q_stride + j
    long m_b_stride, m_h_stride, m_q_stride;
    int mask_f32;                // 1: fp32 mask (added in fp32), 0: bf16 mask (sum rounded to bf16)
    int B, Lq, Lk, H, Hkv, hd;
    float scale;
    int scale_div;               // 1: s / scale (Gemma's "/ math.sqrt(head_dim)"), 0: s * scale (SigLIP)
};
size_t attention_exact_lds(int Lk, int hd);
void attention_exact(hipStream_t s, const ModAttnArgs& a);
// apply_rotary_pos_emb on one projection: x (rows, heads*hd), cos/sin (rows, hd) bf16
void rope_rows(hipStream_t s, const uint16_t* x, const uint16_t* cs, const uint16_t* sn, long rows, int heads, int hd,
               uint16_t* out);

// ---------------------------------------------------------------- misc
// Fused consumer of a projection + residual: if split > 1, h = bf16(bf16(sum_z ws[z] (+bias)) + h)
// (fixed z order) is written back to h first; then out = norm(h): RMSNorm (b == nullptr,
// (1 + w) form) or LayerNorm (b != nullptr).  D <= 4096.
void splitk_res_norm(hipStream_t s, const float* ws, int split, const uint16_t* bias, uint16_t* h, const uint16_t* w,
                     const uint16_t* b, float eps, uint16_t* out, int rows, int D);
void rmsnorm(hipStream_t s, const uint16_t* x, const uint16_t* w, float eps, uint16_t* out, int rows, int D);
void layernorm(hipStream_t s, const uint16_t* x, const uint16_t* w, const uint16_t* b, float eps, uint16_t* out,
               int rows, int D);
void embed_rows(hipStream_t s, const int64_t* ids, int rows, const uint16_t* E, int D, float normalizer,
                int64_t pad_id, uint16_t* out);
// merge (modeling_gemma.py:468-537) + GemmaModel normalizer (:367-368)
// lens (may be null): row b's tokens are ids[b][0 .. lens[b]); the slots past them are padding -- zero rows,
// their ids never looked up (nor counted as <image> tokens)
void merge_embed(hipStream_t s, const int64_t* ids, int B, int L, const uint16_t* E, int D,
                 const uint16_t* img, int n_img_rows, int64_t image_token, int64_t pad_id, float sqrt_h,
                 float normalizer, const uint16_t* embeds_in, int* scan_buf, uint16_t* out,
                 const int* lens = nullptr);
// out[b] = x[b][lens[b] - 1] (rows of D bf16, D % 8 == 0): each sequence's last real token of a ragged batch
void gather_last_rows(hipStream_t s, const uint16_t* x, int B, int L, int D, const int* lens, uint16_t* out);
// sequences per context (pgmi_create's max_batch bound): the 16 rows of the batched decode projections' MFMA tile
constexpr int kMaxRows = 16;
// per-row host values handed to a setter kernel by value (B <= kMaxRows rows): no staging copy, and nothing of
// the host arrays is read after the launch call returns
struct RowInts { int v[kMaxRows]; };
// the ragged step's per-row records: st[b] = {kv_lens.v[b], positions.v[b]}
void set_step_rows(hipStream_t s, StepState* st, const RowInts& kv_lens, const RowInts& positions, int B);
// dst[b] = a.v[b], dst[kMaxRows + b] = b2.v[b] (a ragged prefill's token counts and attended key counts)
void set_row_ints(hipStream_t s, int* dst, const RowInts& a, const RowInts& b2, int B);
void scale_rows(hipStream_t s, const uint16_t* x, long n, float normalizer, uint16_t* out);
void add_rows(hipStream_t s, const uint16_t* x, const uint16_t* y, long n, uint16_t* out);  // bf16(x + y), n % 8 == 0
// qkv: bf16 [B*L][(nh+2nkv)*256], or (split > 1) the fp32 partial slabs ws[split][B*L][...]
void rope_kv_append(hipStream_t s, const uint16_t* qkv, const float* ws, int split, int B, int L, int nh, int nkv,
                    const int64_t* pos, const uint16_t* cosT, const uint16_t* sinT, int max_pos, uint16_t* q_out,
                    uint16_t* kcache, uint16_t* vcache, long kv_b_stride, int kv_start);
void patchify(hipStream_t s, const void* px, int px_is_f32, int B, int C, int H, int W, int P, int Kpad,
              uint16_t* out);
void fill_synthetic(hipStream_t s, uint16_t* dst, long n, uint64_t key, float scale, float offset);
// dst[i] = bf16(src[i]), src fp32 or fp16 (PGMI_DTYPE_F32 / PGMI_DTYPE_F16), round to nearest even
__attribute__((visibility("hidden"))) void convert_to_bf16(hipStream_t s, const void* src, int dtype, long n,
                                                          uint16_t* dst);
void set_step(hipStream_t s, StepState* st, int kv_len, int position);
// step state with the rotary position read on the device: round(pos[0]) of a (B, 1) position tensor
// of dtype PGMI_DTYPE_* (+ 10 = int64, 11 = int32, 12 = float64) -- no host read of a merge's positions
void set_step_dev(hipStream_t s, StepState* st, int kv_len, const void* pos, int dtype);
// an additive mask row set (B rows of n keys, element (b, j) at src[b * b_stride + j], dtype bf16 / fp32)
// -> fp32 [B][ld]
void stage_mask(hipStream_t s, const void* src, int dtype, int B, long b_stride, int n, float* dst, int ld);
// PIL-exact BICUBIC resize of a uint8 HWC RGB image + rescale/normalize -> float32 CHW
// (processing_paligemma.py:13-49); scratch of preprocess_scratch_bytes() on the device
size_t preprocess_scratch_bytes(int H, int W, int out_h, int out_w);
void preprocess(hipStream_t s, const uint8_t* src, int H, int W, int out_h, int out_w, float* out, void* scratch);
void pad_rows(hipStream_t s, const uint16_t* src, int rows, int K, int Kpad, uint16_t* dst);
// nucleus sampling (kernels_sample.hip; inference.py:15-24, :65); scratch of sample_scratch_bytes()
size_t sample_scratch_bytes(int rows, int V);
void sample_top_p(hipStream_t s, const float* x, int rows, int V, float temperature, float top_p, const float* u,
                  void* scratch, int64_t* out, float* kept_mass);


bool gemv_logits_folds(int B);

}  // namespace pgmi
