/*
 * vtamiq_hip.h -- C ABI of libvtamiq_hip.so, the MI355X (gfx950) engine for VTAMIQ's ViT patch-pair forward.
 *
 * The reference (ch-andrei/VTAMIQ) is pure Python/PyTorch and has no FFI of its own; this header is the
 * boundary a maintainer binds with ctypes.  Each entry point names the reference code
 * it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless stated otherwise; the caller (torch) owns all inputs/outputs,
 *     the library owns only packed weights and its workspace;
 *   - all calls are asynchronous on the hipStream_t passed in (void* here so the header needs no HIP include);
 *     no internal synchronisation except where stated, and except ONE wait that any launching call may make: the first time a
 *     process runs the persistent 256x256 GEMM at a new (device, tile grid) -- from vtq_reserve, from the top of a forward, or from
 *     vtq_k_gemm -- its tile schedule (a few KiB) is uploaded on `stream` and the host waits for `stream` before the schedule enters
 *     the process-wide cache, so that every later launch, on whichever stream of that device, finds it complete;
 *   - int return: 0 = ok, non-zero = error; text via vtq_last_error(); no exceptions cross the ABI;
 *   - a handle is not thread-safe: one thread at a time per handle.  Different handles may be used from different threads and on
 *     different streams at the same time; what they share (the schedule cache, each kernel's first-use configuration) is guarded.
 */
#ifndef VTAMIQ_HIP_H
#define VTAMIQ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VTQ_ABI_VERSION 10

/* numerics mode of the dense contractions (fp32 accumulate, fp32 LayerNorm/softmax/residual in all of them).
 * bf16 and fp16 MFMAs run at the same rate on gfx950; fp16 carries 11 significand bits instead of 8 in the range the reference's
 * own GPU path uses for these contractions (torch.cuda.amp.autocast(float16), train.py:602). */
#define VTQ_PREC_BF16   0   /* one bf16 MFMA per product                                                                      */
#define VTQ_PREC_BF16X3 1   /* operands split hi+lo bf16: a_hi*w_hi + a_lo*w_hi + a_hi*w_lo (3 MFMAs)                          */
#define VTQ_PREC_FP16   2   /* one fp16 MFMA per product                                                                      */
#define VTQ_PREC_FP16X3 3   /* operands split hi+lo fp16, 3 MFMAs per product: at the fp32 reference's own noise floor         */
#define VTQ_PREC_FP16X2 4   /* linear layers: activations split hi+lo fp16, weights single fp16 (2 MFMAs per product);         */
                            /* attention (QK^T, PV): the 3-term fp16 form                                                      */
/* 5 is the fp8 EXPERIMENT (BASELINE configs[4]): not a scoring mode and not in this library -- vtq_create rejects it unless the library
 * was built with -DVTQ_WITH_FP8; its constants and entry points live in include/vtamiq_hip_fp8.h. */

/* operand-format code of the per-kernel entry points: MFMAs per product (1 | 2 | 3) + 16 for fp16 planes (0 = bf16):
 *   1 / 17 single plane each; 18 = activation hi/lo planes x single weight plane (fp16 only); 3 / 19 = hi/lo planes for both */
#define VTQ_NUM_BF16   1
#define VTQ_NUM_BF16X3 3
#define VTQ_NUM_FP16   17
#define VTQ_NUM_FP16X2 18
#define VTQ_NUM_FP16X3 19

typedef struct vtq_config {
    int32_t hidden_size;       /* 768 | 1024                (transformer.py:68-98)                    */
    int32_t mlp_dim;           /* 3072 | 4096                                                         */
    int32_t num_heads;         /* 12 | 16 ; head_dim must be 64                                       */
    int32_t num_layers;        /* kept layers               (transformer.py:342-345)                  */
    int32_t patch_dim;         /* 3*16*16 = 768 | 3*8*8 = 192 (ViT-B/8, transformer.py:81-85)         */
    int32_t pos_grid;          /* img_dim / patch: 24 | 48   (transformer.py:411)                     */
    int32_t num_extra_tokens;  /* register tokens           (transformer.py:487-492)                  */
    int32_t num_scales;        /* scale embedding iff > 1   (transformer.py:500)                      */
    int32_t use_layer_scale;   /* ls1/ls2 gamma             (transformer.py:270-271)                  */
    int32_t calibrate;         /* DiffNet on/off            (vtamiq.py:63-69)                         */
    int32_t diff_scale;        /* LayerScale on the CLS diff (vtamiq.py:61)                           */
    int32_t num_rgs;           /* vtamiq.py:34                                                        */
    int32_t num_rcabs;         /* vtamiq.py:35                                                        */
    int32_t ca_hidden;         /* hidden_size / ca_reduction (channel_attention.py:75)                */
    int32_t precision;         /* VTQ_PREC_*                                                          */
    int32_t num_adapters;      /* Adapter pairs per layer (transformer.py:260-269); pair 0 is applied   */
    int32_t options;           /* VTQ_OPT_* bit mask (tests and measurement; 0 = the product path)      */
    int32_t reserved[3];
} vtq_config;

/* vtq_config.options.  The library reads NO environment variable: what rounds 1-3 steered through VTQ_NO_CLS_PRUNE /
 * VTQ_FP8_STATIC_SCALES is an explicit field of the configuration the caller hands over. */
#define VTQ_OPT_FULL_LAST_LAYER   1   /* run the last encoder layer on every token row instead of on the CLS rows only (same result) */
                                      /* (2 belongs to the fp8 experiment: include/vtamiq_hip_fp8.h)                                  */
#define VTQ_OPT_FUSED_LAYERNORM   4   /* LayerNorm inside the residual GEMMs: the out-proj launch also writes LayerNorm 2's operand planes, */
                                      /* the fc2 launch the next layer's LayerNorm 1 planes (csrc/gemm_rowln.hip; hidden 768, 3-term          */
                                      /* formats, no adapters: vtq_create fails otherwise).  Bit-identical scores; measured 1.3 % SLOWER at   */
                                      /* B = 32 than separate LayerNorm launches, hence opt-in                               */

typedef struct vtq_tensor_desc {
    const char*  name;         /* HOST string: the reference's state_dict key          */
    const float* data;         /* DEVICE pointer, fp32, contiguous                                    */
    int64_t      numel;
} vtq_tensor_desc;

typedef struct vtq_engine* vtq_handle;

int         vtq_abi_version(void);
const char* vtq_last_error(void);

/* Replaces VTAMIQ.__init__ / VisionTransformer.__init__ for the inference path (vtamiq.py:27-79). */
int  vtq_create(const vtq_config* cfg, vtq_handle* out);
void vtq_destroy(vtq_handle h);

/* Replaces Module.load_state_dict for the engine: borrows fp32 device tensors for the duration of the call
 * (which synchronises the stream before returning) and packs them to bf16 (hi[,lo]) / fp32 buffers owned by
 * the handle.  Unknown names are an error; every tensor of the configured topology must be present. */
int  vtq_load_weights(vtq_handle h, const vtq_tensor_desc* descs, int32_t n, void* stream);

/* Bytes of device workspace the handle holds for a (B pairs, N patches) call.  A capacity of (B, N) is an upper bound for EVERY workspace
 * buffer of a vtq_forward_varlen call of at most B pairs with at most N patches each (its token rows, patch rows, per-sequence rows,
 * fold partials and per-call tables are all no larger than those of B uniform pairs of N patches): vtq_reserve(h, B, max n) ahead of
 * such calls means none of them allocates.  The same holds for vtq_forward_group_varlen, vtq_encode_reference_varlen and
 * vtq_forward_cached_varlen with B = ceil(sequences / 2) and N = the largest count of any image, the per-call table included. */
size_t vtq_workspace_bytes(vtq_handle h, int32_t B, int32_t N);
/* Grows the workspace ahead of time (hipMalloc happens here, or lazily on the first larger vtq_forward). */
int  vtq_reserve(vtq_handle h, int32_t B, int32_t N);

/* Replaces VTAMIQ.forward (vtamiq.py:94-119): q_out[B] = score of each (ref, dist) pair.
 *   patches_* : [B, N, 3, 16, 16] fp32 contiguous      pos_* : [B, N, 2] fp32 in [0,1)
 *   scales_*  : [B, N] fp32-cast scale ids, or NULL when the model has no scale embedding
 *               (NULL with num_scales > 1 is an error, as in transformer.py:547-548).
 * Every scoring entry of this header (vtq_forward*, vtq_encode_reference*, vtq_forward_cached*) refuses a bad call with no launch, with text
 * that names the entry, and checks in one order: the batch description, which needs no handle (a NULL count array or ref_index, the extents,
 * a count < 1, a ref_index out of range, a NULL rollout_out); the handle (NULL, the fp8 experiment's, a set token trace); NULL tensors and
 * outputs; what a rollout form adds; the scale rule and the weights.  A call that is wrong twice is refused for the earlier reason. */
int  vtq_forward(vtq_handle h,
                 const float* patches_ref, const float* patches_dist,
                 const float* pos_ref, const float* pos_dist,
                 const float* scales_ref, const float* scales_dist,
                 int32_t B, int32_t N, float* q_out, void* stream);

/* vtq_forward on B pairs with DIFFERENT patch counts: pair b has n_patches[b] >= 1 patches in both of its images (n_patches: HOST array
 * of B entries, read before the call returns).  With SN = the sum of n_patches:
 *   patches_* : (SN, 3, P, P) fp32 contiguous -- the pairs' patches one after the other      pos_* : (SN, 2)
 *   scales_*  : (SN) or NULL, under the rule of vtq_forward                                   q_out : B scores
 * q_out[b] has the bits vtq_forward gives for pair b alone (B = 1, N = n_patches[b]) on the same handle, in every numerics mode, with the
 * CLS-only last layer and with VTQ_OPT_FULL_LAST_LAYER; with all n_patches equal the call is bit-identical to vtq_forward.  Sequences
 * (n_patches[b] + T token rows) are packed back to back at their own length, all reference sequences, then all distorted ones; the
 * call's tables (row offsets, lengths, attention block table) are built on the host and uploaded to buffers of THIS handle
 * on `stream` ahead of the first launch.  Asynchronous on `stream` (a second call waits for the previous call's table upload, not for
 * its kernels); vtq_input_errors bits 0 and 1 as vtq_forward.  Workspace: as vtq_forward(B, max n_patches) -- see vtq_workspace_bytes.
 * Refused with vtq_last_error text and no launch: a NULL handle, tensor, n_patches or q_out; B < 1; an n_patches[b] < 1; the fp8
 * experiment's handle; a set token trace buffer (vtq_set_token_trace). */
int  vtq_forward_varlen(vtq_handle h, const float* patches_ref, const float* patches_dist, const float* pos_ref, const float* pos_dist,
                        const float* scales_ref, const float* scales_dist, int32_t B, const int32_t* n_patches, float* q_out, void* stream);

/* VTAMIQ.forward on PRE-EMBEDDED input: Embeddings.forward takes the (B, N, H) branch (transformer.py:534-535) -- what a model built with
 * use_patch_embedding=False is fed, and what the reference does with ANY 3-D `patches` tensor.  feats_*: (B, N, hidden_size) fp32, contiguous; everything
 * else as vtq_forward.  The patch-embedding weights are not used (they must still be loaded: zeros do). */
int  vtq_forward_tokens(vtq_handle h, const float* feats_ref, const float* feats_dist, const float* pos_ref, const float* pos_dist,
                        const float* scales_ref, const float* scales_dist, int32_t B, int32_t N, float* q_out, void* stream);

/* vtq_forward plus the ATTENTION ROLLOUT of the token the score is read from (Abnar & Zuidema): which patches each image's score looked at.
 * With T = 1 + num_extra_tokens, S = T + N, L = num_layers, h = num_heads, t = the consumed token (vtq_set_iqa_token), and P_l[k][b][hd] the
 * S x S matrix softmax(Q K^T / 8) of layer l, head hd, image k (0 = reference, 1 = distorted) of pair b -- exactly vtq_forward_vit's `probs`:
 *     A_l = 1/2 (I + 1/h sum_hd P_l[hd])           rollout[k][b][:] = e_t^T A_L A_{L-1} ... A_1           last_attention[k][b][hd][:] = P_L[k][b][hd][t][:]
 * evaluated as a row vector from the last layer to the first, r <- 1/2 r + 1/(2h) sum_hd r^T P_l[hd]; no S x S matrix is stored.  Tokens
 * first, then the N patches in input order; every value > 0, each rollout row sums to 1.  Nothing else is applied (no renormalisation over
 * patches, no discarding of heads).
 *   rollout_out        : fp32, EXACTLY 2 * B * S floats ([2][B][S]); required
 *   last_attention_out : fp32, EXACTLY 2 * B * h * S floats ([2][B][h][S]); may be NULL
 *   every other argument as vtq_forward / vtq_forward_tokens; q_out has the bits vtq_forward gives.
 * A pair's rollout and last_attention do not depend on the batch it is in.  Asynchronous on `stream`; vtq_input_errors as vtq_forward.
 * The Q / K planes of every layer survive the forward in buffers of their own, reserved by these entries only and grown like the
 * workspace: vtq_rollout_workspace_bytes(h, B, N) bytes on top of vtq_workspace_bytes (about num_layers times the QKV buffer);
 * vtq_workspace_bytes and every other entry are unchanged.  The scores still come from the CLS-only last layer; its Q and K rows are
 * projected in addition, because the probabilities vtq_forward_vit reports are those of the 16-bit Q / K planes, which the tail never forms.
 * Refused with vtq_last_error text and no launch: a NULL handle or rollout_out; B or N < 1; the fp8 experiment's handle; a set token trace
 * buffer (vtq_set_token_trace); a set vtq_debug_stop_after.  vtq_forward_pairwise has no rollout form; the varlen, group and cached entries
 * have one each ("rollout forms" below, behind the one-to-many entries); the ragged rollouts (vtq_forward_varlen_rollout,
 * vtq_forward_group_varlen_rollout ...) take 5-D patches only: pre-embedded ragged input is not offered. */
int  vtq_forward_rollout(vtq_handle h, const float* patches_ref, const float* patches_dist, const float* pos_ref, const float* pos_dist,
                         const float* scales_ref, const float* scales_dist, int32_t B, int32_t N, float* q_out, float* rollout_out,
                         float* last_attention_out, void* stream);
int  vtq_forward_rollout_tokens(vtq_handle h, const float* feats_ref, const float* feats_dist, const float* pos_ref, const float* pos_dist,
                                const float* scales_ref, const float* scales_dist, int32_t B, int32_t N, float* q_out, float* rollout_out,
                                float* last_attention_out, void* stream);
/* Bytes of the extra device workspace a vtq_forward_rollout call of (B pairs, N patches) holds beside vtq_workspace_bytes(h, B, N).  The
 * rollout forms of the other entries hold vtq_rollout_workspace_bytes(h, ceil(sequences / 2), N), the variable-length ones with N = the
 * largest count of any image -- an upper bound for every buffer of such a call, as vtq_workspace_bytes is for the base entry. */
size_t vtq_rollout_workspace_bytes(vtq_handle h, int32_t B, int32_t N);

/* Pairwise items (train.predict, train.py:281-301: two model calls sharing the reference image): patches/pos/scales are HOST
 * arrays of 3 DEVICE pointers {ref, dist1, dist2}, each as in vtq_forward (scales may be NULL); the reference image is
 * encoded ONCE (3B sequences instead of 4B).  q_out[2B]: q_out[b] = score(ref_b, dist1_b), q_out[B + b] = score(ref_b, dist2_b);
 * bit-identical to two vtq_forward calls. */
int  vtq_forward_pairwise(vtq_handle h, const float* const* patches, const float* const* pos, const float* const* scales,
                          int32_t B, int32_t N, float* q_out, void* stream);

/* vtq_forward_pairwise on PRE-EMBEDDED input (the (B, N, H) branch of Embeddings.forward, as vtq_forward_tokens): feats = HOST array of 3 DEVICE
 * pointers {ref, dist1, dist2}, each (B, N, hidden_size) fp32 contiguous.  Bit-identical to two vtq_forward_tokens calls. */
int  vtq_forward_pairwise_tokens(vtq_handle h, const float* const* feats, const float* const* pos, const float* const* scales,
                                 int32_t B, int32_t N, float* q_out, void* stream);

/* VisionTransformerBackbone.forward_vit (backbone.py:54-60, transformer.py:628-641, 363-378) on B SINGLE images: the encoder with no head.
 *   in       (B, N, 3, P, P) fp32 patches, or (tokens_in != 0) (B, N, hidden_size) pre-embedded rows; pos (B, N, 2); scales (B, N) or NULL
 *            (required when num_scales > 1) -- as one image of vtq_forward / vtq_forward_tokens.
 *   Rows per sequence: R = T = 1 + num_extra_tokens (all_tokens == 0, tokens_only=True) or R = S = N + T (all_tokens != 0).
 *   out      (B, R, hidden_size) fp32: encoder_norm of the last layer's rows.  Required.
 *   states   NULL, or (L, B, R, hidden_size) fp32: the residual stream after each layer, before encoder_norm (no embedding output).
 *   probs    NULL, or (L, B, num_heads, S, S) fp32: each layer's attention probabilities softmax(Q K^T / sqrt(64)).
 * The last layer always runs on every row (the result of VTQ_OPT_FULL_LAST_LAYER); the adapter pair 0 applies as in vtq_forward.
 * Caller-owned device buffers, asynchronous on `stream`; positions outside [0, 1) are recorded in vtq_input_errors bit 0, a
 * non-finite output value in bit 1.  Refused: the fp8 experiment's handle, a NULL out / in / pos, B or N < 1. */
int  vtq_forward_vit(vtq_handle h, const float* in, int32_t tokens_in, const float* pos, const float* scales, int32_t B, int32_t N,
                     int32_t all_tokens, float* out, float* states, float* probs, void* stream);

/* ---- one-to-many scoring: M distorted images over G references, every reference encoded ONCE -------------------------------------------
 * Full-reference data holds a few references with many distorted versions each; these entries encode G + M (or M) sequences where
 * vtq_forward on the expanded pairs encodes 2 M.  Distorted image m is scored against reference ref_index[m]; ref_index is a HOST array of M
 * entries in [0, G), in any order, with repeats and unused references allowed, read before the call returns and uploaded to a buffer of THIS
 * handle on `stream` ahead of the first launch (through the handle's pinned image, as vtq_forward_varlen's tables: a second call waits for the
 * previous call's upload, not for its kernels).
 * The contract of all of them: q_out[m] has the bits vtq_forward gives for the single pair (reference ref_index[m], distorted m) (B = 1) on the
 * same handle, in every numerics mode, with the CLS-only last layer and with VTQ_OPT_FULL_LAST_LAYER -- a score never depends on what else is
 * in the batch.  vtq_input_errors bits 0 and 1 as vtq_forward; a NaN distorted image makes only its own score NaN, a NaN reference exactly
 * the scores that point at it.  Asynchronous on `stream`.  Workspace: as vtq_forward with ceil(sequences / 2) pairs (vtq_workspace_bytes).
 * Refused with vtq_last_error text and no launch: a NULL ref_index (where one is taken); G, M or N < 1; a ref_index[m] outside [0, G); a NULL
 * handle, tensor or output; the fp8 experiment's handle; a set token trace buffer (vtq_set_token_trace).
 *
 * vtq_forward_group: references and distorted images in one batch of G + M sequences.
 *   patches_ref : [G, N, 3, P, P] fp32 contiguous      pos_ref  : [G, N, 2]      scales_ref  : [G, N] or NULL, under the rule of vtq_forward
 *   patches_dist: [M, N, 3, P, P]                      pos_dist : [M, N, 2]      scales_dist : [M, N] or NULL
 *   ref_index   : HOST int32 [M]                       q_out    : [M] fp32
 * The two patch tensors are read where they lie (no device-side concatenation). */
int  vtq_forward_group(vtq_handle h, const float* patches_ref, const float* patches_dist, const float* pos_ref, const float* pos_dist,
                       const float* scales_ref, const float* scales_dist, int32_t G, int32_t M, int32_t N, const int32_t* ref_index,
                       float* q_out, void* stream);
/* vtq_forward_group on PRE-EMBEDDED input (as vtq_forward_tokens): feats_ref [G, N, hidden_size], feats_dist [M, N, hidden_size]. */
int  vtq_forward_group_tokens(vtq_handle h, const float* feats_ref, const float* feats_dist, const float* pos_ref, const float* pos_dist,
                              const float* scales_ref, const float* scales_dist, int32_t G, int32_t M, int32_t N, const int32_t* ref_index,
                              float* q_out, void* stream);
/* The reference cache, for distorted images that arrive after their reference.  vtq_encode_reference encodes G SINGLE images
 *   in : [G, N, 3, P, P] fp32 patches, or (tokens_in != 0) [G, N, hidden_size] pre-embedded rows;  pos : [G, N, 2];  scales : [G, N] or NULL
 * and writes ref_rows : [G, hidden_size] fp32 (exactly G * hidden_size floats, caller-owned: they outlive any later call and any workspace
 * growth) = the residual-stream row of the consumed token (vtq_set_iqa_token) after the last layer, BEFORE encoder_norm -- what the
 * difference behind vtq_forward reads, so a later vtq_forward_cached does the same arithmetic.  The last layer runs in the form vtq_forward
 * picks (the CLS-only tail unless VTQ_OPT_FULL_LAST_LAYER or adapters force the full layer), not vtq_forward_vit's always-full one.  A
 * non-finite value in a row raises vtq_input_errors bit 1.  The rows belong to this handle's numerics mode, weights, options and consumed
 * token: the caller keeps track of those (vtamiq_amd.ReferenceFeatures does). */
int  vtq_encode_reference(vtq_handle h, const float* in, int32_t tokens_in, const float* pos, const float* scales, int32_t G, int32_t N,
                          float* ref_rows, void* stream);
/* vtq_forward_cached encodes the M distorted images only and takes the reference rows from ref_rows through ref_index:
 *   ref_rows : [G, hidden_size] fp32 of vtq_encode_reference (read only: rows ref_index[m], nothing else)
 *   in       : [M, N, 3, P, P] or (tokens_in != 0) [M, N, hidden_size];  pos : [M, N, 2];  scales : [M, N] or NULL;  q_out : [M] fp32
 * N need not be the N the references were encoded with: nothing behind the encoder depends on it. */
int  vtq_forward_cached(vtq_handle h, const float* ref_rows, int32_t G, const float* in, int32_t tokens_in, const float* pos,
                        const float* scales, int32_t M, int32_t N, const int32_t* ref_index, float* q_out, void* stream);

/* ---- one-to-many scoring on images of DIFFERENT patch counts: the entries above with vtq_forward_varlen's layout ----------------------------
 * Mixed-size full-reference data: a few references with many distorted versions each, patch counts differing between images.  Every image
 * has its own count >= 1 (HOST arrays, read before the call returns); a distorted image's count need NOT equal its reference's: nothing
 * behind the encoder depends on it.  Tensors as in vtq_forward_varlen, the images' patches one after the other, 5-D patches only:
 *   patches_ref : (sum n_ref, 3, P, P) fp32 contiguous      pos_ref  : (sum n_ref, 2)       scales_ref  : (sum n_ref) or NULL, vtq_forward's rule
 *   patches_dist: (sum n_dist, 3, P, P)                     pos_dist : (sum n_dist, 2)      scales_dist : (sum n_dist) or NULL
 *   n_ref : HOST int32 [G]    n_dist : HOST int32 [M]    ref_index : HOST int32 [M], entries in [0, G)    q_out : [M] fp32    ref_rows : [G, hidden_size]
 * Sequences (count + T token rows) are packed back to back at their own length, all G reference sequences, then all M distorted ones.  The
 * call's table (row offsets, lengths, ref_index, attention block table) is built on the host and uploaded ONCE through the handle's pinned
 * image on `stream` ahead of the first launch; a second call waits for the previous call's upload, not for its kernels.  Asynchronous on
 * `stream`.  In every numerics mode, with the CLS-only last layer and with VTQ_OPT_FULL_LAST_LAYER:
 *   - ref_rows[g] of vtq_encode_reference_varlen has the bits vtq_encode_reference gives reference g alone (G = 1, N = n_patches[g]);
 *   - q_out[m] of vtq_forward_cached_varlen has the bits vtq_forward_cached gives that image alone (M = 1, N = n_patches[m]) against the same rows;
 *   - q_out[m] of vtq_forward_group_varlen has the bits of that chain: reference ref_index[m] encoded alone, then distorted image m scored
 *     alone against it -- where n_ref[ref_index[m]] == n_dist[m], the bits of vtq_forward on the single pair;
 *   - with all counts equal a call is bit-identical to the uniform entry.
 * A NaN distorted image makes only its own score NaN, a NaN reference exactly the scores that point at it; vtq_input_errors bits 0 and 1
 * as vtq_forward.  Workspace: as vtq_forward with ceil((G + M) / 2) pairs (ceil(G / 2), ceil(M / 2) for the single-image entries) of the
 * largest count -- see vtq_workspace_bytes.
 * Refused with vtq_last_error text that names the entry and the offending argument, and no launch: a NULL count array, ref_index, handle,
 * tensor or output; G or M < 1; a count < 1; a ref_index[m] outside [0, G); the fp8 experiment's handle; a set token trace buffer
 * (vtq_set_token_trace).  The checks of the batch description need no device and come first. */
int  vtq_forward_group_varlen(vtq_handle h, const float* patches_ref, const float* patches_dist, const float* pos_ref, const float* pos_dist,
                              const float* scales_ref, const float* scales_dist, int32_t G, int32_t M, const int32_t* n_ref,
                              const int32_t* n_dist, const int32_t* ref_index, float* q_out, void* stream);
int  vtq_encode_reference_varlen(vtq_handle h, const float* patches, const float* pos, const float* scales, int32_t G, const int32_t* n_patches,
                                 float* ref_rows, void* stream);
int  vtq_forward_cached_varlen(vtq_handle h, const float* ref_rows, int32_t G, const float* patches, const float* pos, const float* scales,
                               int32_t M, const int32_t* n_patches, const int32_t* ref_index, float* q_out, void* stream);

/* ---- rollout forms of the variable-length and one-to-many entries ---------------------------------------------------------------------------
 * Each is its base entry -- the same arguments, the same q_out / ref_rows bits, the same refusals -- plus the rollout of vtq_forward_rollout
 * for every sequence the call ENCODES, in the same launch sequence: `float* rollout_out, float* last_attention_out` stand before `stream`.
 * A sequence's maps depend on its own image alone: they have the bits vtq_forward_rollout gives for a single pair (B = 1) holding that image
 * with the same patch count, on the reference side for a reference and on the distorted side for a distorted image.  A NaN image makes
 * exactly its own maps NaN.  h = num_heads, S = T + N; S_j = T + the count of sequence j.
 *   uniform (vtq_forward_group_rollout, _tokens):  rollout_out : fp32, EXACTLY (G + M) * S floats ([G + M][S], the references first)
 *                                                  last_attention_out : fp32, EXACTLY (G + M) * h * S floats ([G + M][h][S]); may be NULL
 *   vtq_encode_reference_rollout:                  rollout_out : fp32, EXACTLY G * S floats ([G][S])
 *                                                  last_attention_out : fp32, EXACTLY G * h * S floats ([G][h][S]); may be NULL
 *   vtq_forward_cached_rollout:                    rollout_out : fp32, EXACTLY M * S floats ([M][S])
 *                                                  last_attention_out : fp32, EXACTLY M * h * S floats ([M][h][S]); may be NULL
 *                                                  (the cached references are not encoded: their maps come from vtq_encode_reference_rollout)
 *   variable-length (vtq_forward_varlen_rollout, vtq_forward_group_varlen_rollout, vtq_encode_reference_varlen_rollout,
 *   vtq_forward_cached_varlen_rollout), with R = the sum of S_j over the call's sequences in call order -- vtq_forward_varlen_rollout: all B
 *   reference sequences, then all B distorted ones; the group form: the G references, then the M distorted images:
 *                                                  rollout_out : fp32, EXACTLY R floats: sequence j's S_j values at the sum of S_i, i < j
 *                                                  last_attention_out : fp32, EXACTLY h * R floats: sequence j's [h][S_j] block at h times
 *                                                  that offset; may be NULL
 * Both are written by the call's last launches on `stream` (no copy); nothing outside the stated extents is written.  Extra workspace: see
 * vtq_rollout_workspace_bytes.  Refused with vtq_last_error text that names the entry, and no launch: everything the base entry refuses (bad
 * counts and ref_index, the fp8 experiment's handle, a set token trace buffer ...); a NULL rollout_out (with the batch description, ahead of
 * the handle); a set vtq_debug_stop_after; more than 65535 sequences. */
int  vtq_forward_varlen_rollout(vtq_handle h, const float* patches_ref, const float* patches_dist, const float* pos_ref, const float* pos_dist,
                                const float* scales_ref, const float* scales_dist, int32_t B, const int32_t* n_patches, float* q_out,
                                float* rollout_out, float* last_attention_out, void* stream);
int  vtq_forward_group_rollout(vtq_handle h, const float* patches_ref, const float* patches_dist, const float* pos_ref, const float* pos_dist,
                               const float* scales_ref, const float* scales_dist, int32_t G, int32_t M, int32_t N, const int32_t* ref_index,
                               float* q_out, float* rollout_out, float* last_attention_out, void* stream);
int  vtq_forward_group_rollout_tokens(vtq_handle h, const float* feats_ref, const float* feats_dist, const float* pos_ref, const float* pos_dist,
                                      const float* scales_ref, const float* scales_dist, int32_t G, int32_t M, int32_t N, const int32_t* ref_index,
                                      float* q_out, float* rollout_out, float* last_attention_out, void* stream);
int  vtq_encode_reference_rollout(vtq_handle h, const float* in, int32_t tokens_in, const float* pos, const float* scales, int32_t G, int32_t N,
                                  float* ref_rows, float* rollout_out, float* last_attention_out, void* stream);
int  vtq_forward_cached_rollout(vtq_handle h, const float* ref_rows, int32_t G, const float* in, int32_t tokens_in, const float* pos,
                                const float* scales, int32_t M, int32_t N, const int32_t* ref_index, float* q_out, float* rollout_out,
                                float* last_attention_out, void* stream);
int  vtq_forward_group_varlen_rollout(vtq_handle h, const float* patches_ref, const float* patches_dist, const float* pos_ref, const float* pos_dist,
                                      const float* scales_ref, const float* scales_dist, int32_t G, int32_t M, const int32_t* n_ref,
                                      const int32_t* n_dist, const int32_t* ref_index, float* q_out, float* rollout_out, float* last_attention_out,
                                      void* stream);
int  vtq_encode_reference_varlen_rollout(vtq_handle h, const float* patches, const float* pos, const float* scales, int32_t G,
                                         const int32_t* n_patches, float* ref_rows, float* rollout_out, float* last_attention_out, void* stream);
int  vtq_forward_cached_varlen_rollout(vtq_handle h, const float* ref_rows, int32_t G, const float* patches, const float* pos, const float* scales,
                                       int32_t M, const int32_t* n_patches, const int32_t* ref_index, float* q_out, float* rollout_out,
                                       float* last_attention_out, void* stream);

/* Input check.  The reference raises (IndexError / device assert) when a position lies outside [0, 1)
 * (transformer.py:417-421); vtq_forward clamps such an index into the table instead of gathering out of bounds and records it.
 * Bit 0: a position coordinate with floor(pos * pos_grid) outside [0, pos_grid) or NaN (each coordinate is clamped to cell 0 or
 * pos_grid - 1 on its own), or a NaN scale id (the reference's clamp(scale, 0, num_scales - 1) keeps a NaN, whose index then raises;
 * here it takes scale-table row 1).  Every other scale id, +-inf included, is clamped as the reference clamps it and is no error.
 * Bit 1: the CLS difference of some pair was not finite -- an operand left its format's range upstream (the fp16 operand modes
 * carry |v| <= 65504; VTQ_PREC_BF16X3 has the fp32 range), or the inputs / weights held inf / NaN.
 * (Bit 2 is raised by the fp8 experiment only: include/vtamiq_hip_fp8.h.)
 * This call synchronises `stream`, returns the flags accumulated since the last call and clears them. */
int  vtq_input_errors(vtq_handle h, int32_t* flags, void* stream);

/* Which token row of the encoder output the head consumes: VTAMIQ.token_num (vtamiq.py:57, 107-108: "can be CLS token or
 * extra_token").  0 = CLS (the reference's and this library's default), 1 .. num_extra_tokens = a register token.  Applies to every
 * later vtq_forward / vtq_forward_pairwise; an index outside the model's tokens is refused (the reference would read a PATCH row). */
int  vtq_set_iqa_token(vtq_handle h, int32_t token);

/* Debug tap: when buf != NULL, every later vtq_forward also writes the pre-final-LN token rows after the
 * embedding and after each layer: buf[(L+1)][2B][T][H] fp32 (ref sequences first).  Mirrors
 * vit_config["return_layers"] (transformer.py:369-372, 632-636). */
int  vtq_set_token_trace(vtq_handle h, float* buf);
/* Test hooks for localising a divergence: leave the encoder after stage `layer * 7 + k` of the NEXT forwards (k = 0 LayerNorm 1,
 * 1 QKV, 2 attention, 3 out-proj, 4 LayerNorm 2, 5 fc1, 6 fc2; -1 = run everything; the scores of such a forward are
 * meaningless), and borrow the workspace: x = fp32 residual stream [rows, H], lnbuf = LayerNorm / attention output planes,
 * big = QKV / fc1 output planes, in the layouts DESIGN.md section 3 gives for the engine's precision. */
/* Measurement hook: how the pipelined attention kernel's persistent workgroups walk the (sequence, head, 256-row block) items -- 0 (default) XCD-strided:
 * the workgroups of an XCD take the blocks of the same few (sequence, head) pairs side by side, so a pair's K / V tiles are fetched once per XCD;
 * 1: the round-3 walk (consecutive blocks per workgroup; paired when a pair has two blocks).  Same results either way. */
int  vtq_debug_attention_map(int32_t m);
/* Measurement hook for launches on CU-masked streams (hipExtStreamCreateWithCUMask; tools/cu_partition.py): size the persistent grids of
 * the following launches for the CUs such a stream owns -- the 256x256 GEMM for `gemm_cus_per_xcd` workgroups on each of the 8 XCDs (its tile
 * schedule is rebuilt for that grid), the pipelined attention kernel for `attention_cus` CUs.  0 = the whole device (the default).  Process-wide;
 * results never depend on it. */
int  vtq_debug_cu_partition(int32_t gemm_cus_per_xcd, int32_t attention_cus);
/* Which CUs does a stream own?  Launches `nblocks` workgroups that hold a whole CU each (144 KiB of LDS) for ~spin_us microseconds;
 * out[2 b] = XCC id, out[2 b + 1] = HW_ID register (SE / SH / CU fields) of workgroup b.  out: 2 * nblocks uint32 of device memory. */
int  vtq_debug_cu_map(uint32_t* out, int32_t nblocks, int32_t spin_us, void* stream);
int  vtq_debug_stop_after(vtq_handle h, int32_t stage);
int  vtq_debug_buffers(vtq_handle h, void** x, void** lnbuf, void** big, int64_t* rows);
/* Retired: the GEMM clock-stamp diagnostic build no longer exists.  Ignores its arguments, does nothing and returns 0; the entry point
 * stays until the next ABI change. */
int  vtq_debug_gemm_diag(void* buf, int32_t shadow);
/* Which of the two fused-attention kernels vtq_k_attention and the engine launch (process-wide; tests and measurement):
 * 0 = the 4-wave kernel, 1 = the 8-wave software-pipelined kernel, 2 = split (the pipelined kernel on the full 256-row query blocks, the
 * 4-wave kernel on the few rows behind them: S = 521, the reference-default topology), -1 = the library's rule (the pipelined kernel for
 * the 3-term formats when its 256-row blocks fill the chip; split when S is at most 64 rows past a multiple of 256).  Every form
 * computes the same arithmetic in the same order per query row: outputs are bit-identical. */
int  vtq_debug_attention_variant(int32_t variant);
/* Which tile shape vtq_k_gemm and the engine's GEMM launches use (process-wide; tests and measurement): -1 = the library's rule
 * (vtq_k_gemm_tile_rule), 0 = the persistent 256x256 kernel; one workgroup per tile (csrc/gemm_st.hip): 1 = 64x64 tiles with an operand
 * ring of 3, 2 = 64x64 tiles with a ring of 2 (two workgroups per CU), 3 = 128x128 tiles.  Every shape gives every output element the same MFMA sequence and epilogue arithmetic: outputs are bit-identical. */
int  vtq_debug_gemm_variant(int32_t variant);
/* Host-only: the tile shape the library's rule gives an (M, N, K) launch in operand format num (VTQ_NUM_*); -1 = bad format code. */
int  vtq_k_gemm_tile_rule(int32_t M, int32_t N, int32_t K, int32_t num);
/* Host-only: which kernel the library's rule gives nseq sequences of pitch S_pad, hidden size H, operand format num (VTQ_NUM_*) on a
 * device with `cus` compute units: 2 = split, 1 = pipelined, 0 = 4-wave, -1 = bad format code. */
int  vtq_k_attention_rule(int32_t nseq, int32_t S_pad, int32_t H, int32_t num, int32_t cus);

/* The practical ceiling of the matrix pipe on this device (csrc/mfma_stream.hip; bench.py roofline.practical_peak_tflops_measured_here): a bare
 * stream of back-to-back mfma_f32_16x16x32 on register operands on every CU for >= timed_s seconds after >= warm_s seconds of the same
 * load (each <= 30).  f16: 0 = bf16, 1 = fp16 operands; data: 0 = the operand bits of a 3-term product (hi x hi, hi x lo, lo x hi of
 * gaussian planes), 1 = zeros (the issue limit), 2 = uniform random.  *tflops = MFMA-issue TFLOP/s, *ghz (may be NULL) = the clock it
 * implies.  Blocks the calling thread; measurement only. */
int  vtq_debug_mfma_stream(int32_t f16, int32_t data, double warm_s, double timed_s, double* tflops, double* ghz, void* stream);

/* ---- measurement: per-kernel-class HIP-event timing on the launch stream ------------------------------ */
#define VTQ_K_CONVERT  0
#define VTQ_K_PATCH    1   /* patch-embedding GEMM + pos/scale gather epilogue */
#define VTQ_K_LN       2
#define VTQ_K_QKV      3
#define VTQ_K_ATTN     4
#define VTQ_K_OUTPROJ  5
#define VTQ_K_FC1      6
#define VTQ_K_FC2      7
#define VTQ_K_HEAD     8
#define VTQ_K_COUNT    9
/* mask: bit k set = bracket every launch of class k with hipEvents (0 disables). */
int  vtq_profile_enable(vtq_handle h, uint32_t class_mask);
/* Synchronises the recorded events; ms_sum[k], launches[k] for k < VTQ_K_COUNT (HOST arrays); resets. */
int  vtq_profile_collect(vtq_handle h, double* ms_sum, int64_t* launches);

/* ---- per-kernel entry points (unit tests call these through the same ABI) -----------------------------
 * Every comment below states the EXTENT of each pointer argument: what a caller must allocate, what the entry may read and what it writes.
 * Nothing outside the stated extent is written, and no byte outside it influences a result; tests/test_gpu_footprint.py pins both with guard
 * bands around buffers of exactly these sizes.  A call with an argument documented as invalid returns non-zero and launches nothing.
 * Strides and pitches are in ELEMENTS of the buffer's type. */
/* fp32 [numel] -> 16-bit planes (f16: 0 = bf16, 1 = fp16): dst (hi) and, when planes == 2, dst + plane_stride (lo).  numel % 4 == 0.
 * Reads src[0, numel); writes numel elements per plane; elements [numel, plane_stride) between the planes are not touched. */
int  vtq_k_split(const float* src, void* dst, int64_t plane_stride, int64_t numel, int32_t f16, int32_t planes, void* stream);

/* C[M,N] = A[M,K] * W[N,K]^T (+epilogue); A/W are 16-bit planes as above, format `num` = VTQ_NUM_*; M%256==0, N%256==0, N <= 4096,
 * K%128==0 (one MFMA per product) or K%64==0, lda%16==0, ldo%8==0 -- for every tile shape (vtq_debug_gemm_variant): refused otherwise.
 *   A      activation planes (1, or 2 for the 2- / 3-term formats) of [M][lda], a_plane apart: columns [0, K) of rows [0, M) are read, the
 *          columns [K, lda) and the space between planes are not;
 *   W      weight planes (2 for the 3-term formats, else 1) of [N][K], w_plane apart;   bias fp32 [N];   gamma fp32 [N] or NULL;
 *   x_f32  fp32 [M][N] contiguous, read and written by epilogue 2 only;
 *   out16  planes as the activations of `num`, [M][ldo], o_plane apart, written by epilogues 0 / 1 only: columns [0, N) of rows [0, M);
 *          columns [N, ldo) and the space between planes are not touched.
 *   epilogue 0: out16  = acc + bias                 (1 or 2 planes, as the activations of `num`)
 *            1: out16  = gelu_erf(acc + bias)                              (transformer.py:212-215)
 *            2: x_f32 += gamma * (acc + bias)   (gamma NULL = 1)           (transformer.py:279,284) */
int  vtq_k_gemm(const void* A, int64_t a_plane, int32_t lda, const void* W, int64_t w_plane,
                int32_t M, int32_t N, int32_t K, int32_t num, int32_t epilogue,
                const float* bias, const float* gamma, float* x_f32,
                void* out16, int64_t o_plane, int32_t ldo, void* stream);

/* Whole-row residual GEMM with LayerNorm in its epilogue (csrc/gemm_rowln.hip; N = 768, num = VTQ_NUM_BF16X3 | VTQ_NUM_FP16X3, M % 128 == 0,
 * K % 32 == 0, K >= 128, lda % 8 == 0).  A: 2 planes of [M][lda] (columns [0, K) read), W: 2 planes of [768][K]; bias / gamma / ln_w / ln_b
 * fp32 [768]; x_f32 [M][768] and the 2 planes out16 [M][768] (o_plane apart): rows [0, M) only -- rows behind M of a taller buffer are
 * neither read nor written:
 *     x_f32[M, 768] += gamma * (A[M, K] * W[768, K]^T + bias)          (out-proj / fc2 + LayerScale + residual, transformer.py:279, 284)
 *     out16 planes   = LayerNorm(x_f32; ln_w, ln_b, eps 1e-6)           (the NEXT block's attention_norm / ffn_norm, transformer.py:276, 281)
 * in one launch: the workgroup that owns a 128-row panel owns whole rows.  ln_w == NULL: no LayerNorm output (the x update only).
 * x_f32 is bit-identical to vtq_k_gemm epilogue 2, out16 to vtq_k_layernorm applied to it. */
int  vtq_k_gemm_rowln(const void* A, int64_t a_plane, int32_t lda, const void* W, int64_t w_plane, int32_t M, int32_t K, int32_t num,
                      const float* bias, const float* gamma, float* x_f32, const float* ln_w, const float* ln_b,
                      void* out16, int64_t o_plane, void* stream);

/* HOST-only: the persistent schedule vtq_k_gemm uses for an [M, N] output (M, N multiples of 256) with K columns and `wplanes`
 * weight planes: out[0..256] = begin offsets of the 256 workgroups' lists (out[256] = total length), then the lists:
 * entry = (tile << 2) | kind with tile = row_tile * (N/256) + col_tile, kind 0 = 256x256 tile, 1 / 2 = its top / bottom 128 rows.
 * Returns the total length (writes at most cap entries; out may be NULL), or -1 on a bad shape.  No GPU needed. */
int  vtq_k_gemm_schedule(int32_t M, int32_t N, int32_t K, int32_t wplanes, int32_t* out, int32_t cap);

/* LayerNorm(eps=1e-6) rows of x[rows, H] fp32 -> 16-bit planes (transformer.py:253-254, 276, 281).  H = 768 | 1024; w, b fp32 [H]; out:
 * `planes` planes of [rows][H], o_plane apart; elements [rows * H, o_plane) between the planes are not touched. */
int  vtq_k_layernorm(const float* x, const float* w, const float* b, void* out, int64_t o_plane,
                     int32_t rows, int32_t H, int32_t f16, int32_t planes, void* stream);

/* softmax(Q K^T / sqrt(64)) V per (sequence, head) on the packed qkv[rows, 3H] planes (num = VTQ_NUM_* with 1 or 3 terms);
 * sequences are S_pad rows apart, keys >= S are masked; out[rows, H] planes, heads merged (transformer.py:153-166).
 * S_pad - 64 < S <= S_pad (a pitch that leaves a whole 64-key tile empty is refused).
 *   qkv  planes of [rows][3H], `plane` apart, rows >= nseq * S_pad + (ceil128(S_pad) - S_pad): the kernels load whole 128-row query blocks
 *        and 64-key tiles, so up to 127 rows BEHIND the last sequence are read (S_pad % 128 == 1; the engine allocates 128).  They must
 *        be readable; their values -- zero, NaN or anything else -- reach no output, and neither do rows [S, S_pad) of a sequence as
 *        keys or the next sequence's rows (masked scores are replaced, masked V rows zeroed before use).
 *   out  planes of [nseq * S_pad][H], o_plane apart: EVERY row [0, nseq * S_pad) is stored -- rows [S, S_pad) of a sequence hold the
 *        attention of those pad rows' own queries over the keys < S -- and nothing at or behind row nseq * S_pad. */
int  vtq_k_attention(const void* qkv, int64_t plane, void* out, int64_t o_plane,
                     int32_t nseq, int32_t S, int32_t S_pad, int32_t H, int32_t num, void* stream);

/* vtq_k_attention over nseq sequences of DIFFERENT lengths packed back to back (csrc/attention_varlen.hip): sequence j is the seq_len[j] >= 1
 * rows from row sum_{i<j} seq_len[i] (seq_len: HOST array); with R = the sum of all lengths:
 *   qkv  planes of [rows][3H], `plane` apart, rows >= R + 127: the kernel loads whole 128-row query blocks and 64-key tiles from a
 *        sequence's first row, so up to 127 rows BEHIND row R are read.  They must be readable; their values -- zero, NaN, inf --
 *        reach no output, and neither do another sequence's rows (masked scores are replaced, masked V rows zeroed before use).
 *   out  planes of [R][H], o_plane apart: rows [0, R) are stored, nothing at or behind row R.
 * The rows of sequence j are bit-identical to vtq_k_attention(nseq = 1, S = S_pad = seq_len[j]) on that sequence's rows.  num: VTQ_NUM_*
 * with 1 or 3 terms.  A test entry: it uploads its block table to a temporary and waits for `stream` before returning. */
int  vtq_vl_attention(const void* qkv, int64_t plane, void* out, int64_t o_plane, int32_t nseq, const int32_t* seq_len, int32_t H, int32_t num,
                      void* stream);
/* HOST-only: the block table of vtq_vl_attention / vtq_forward_varlen for these lengths -- one entry of 4 ints per workgroup, in work-id
 * order: {first row of the sequence, its length, 128-row query block, head}; the blocks of one (sequence, head) are consecutive work
 * ids (the kernel keeps consecutive ids on one XCD: they share K / V in its L2).  Writes at most cap entries (out may be NULL); returns
 * the number of entries = H / 64 * sum_j ceil(seq_len[j] / 128), or -1 on a bad argument.  No GPU needed. */
int  vtq_vl_attention_blocks(int32_t nseq, const int32_t* seq_len, int32_t H, int32_t* out, int32_t cap);

/* Attention probabilities of every (sequence, head) on the same qkv planes as vtq_k_attention (num = VTQ_NUM_* with 1 or 3 terms):
 * probs[nseq][H / 64][S][S] fp32 = softmax(Q K^T / sqrt(64)) over the keys < S of each sequence; q_log2 != 0 (3-term formats only): Q
 * already carries 1/sqrt(64) * log2(e), as the engine's query projection does in those formats.  Reads only rows [s * S_pad, s * S_pad + S)
 * of sequence s (qkv: planes of nseq * S_pad rows suffice); writes exactly nseq * (H / 64) * S * S floats. */
int  vtq_k_attention_probs(const void* qkv, int64_t plane, float* probs, int32_t nseq, int32_t S, int32_t S_pad, int32_t H, int32_t num,
                           int32_t q_log2, void* stream);

/* One skinny linear stage on the MFMA pipe (CLS tail of the last layer, DiffNet head): out[R, N] = act[R, K] * W[N, K]^T + bias,
 * operands as 16-bit planes in format `num` (VTQ_NUM_*): xa [planes][>= ceil64(R)][ldx], W [planes][ceil16(N)][K], K % 32 == 0.
 *   epi 0 plain | 1 gelu_erf | 2 prelu(*post_slope) | 3 res + gamma * v (gamma NULL = 1) | 4 res + aux * sigmoid(v) |
 *       5 relu for columns >= nsplit (RCAB conv with the channel-attention squeeze folded in, channel_attention.py:45, 58-61)
 * Outputs: y fp32 [R][ldy], columns [0, ycols) (may be NULL); ya: 16-bit planes of columns [pcol0, N), stored at column
 * c - pcol0, as prelu(value, *next_slope) when next_slope != NULL (may be NULL).
 * Extents.  xa: rows [0, ceil64(R)) x columns [0, K) are read (ldx % 8 == 0); rows >= R must be readable, their values reach no output.
 * W: rows [0, ceil16(N)) are read; rows >= N likewise.  Columns of xa and W that only pad K to a multiple of 32 must be ZERO (they are
 * multiplied).  bias, gamma fp32 [N]; res, aux fp32 [R][ldr], columns [0, N) (epilogues 3 / 4); the slopes one float each.
 * y: rows [0, R) x columns [0, ycols) are written (ldy % 4 == 0 unless ycols < 4), columns [ycols, ldy) are not.  ya: activation planes
 * of [R][ldya], ya_plane apart, pcol0 % 4 == 0, ldya % 4 == 0, ldya >= ceil4(N - pcol0): rows [0, R) x columns [0, ceil4(N - pcol0)) are
 * written, the columns >= N - pcol0 among them as zeros (the consumer's K padding); rows >= R are not. */
int  vtq_k_skinny_linear(const void* xa, int64_t xa_plane, int32_t ldx, const void* W, int64_t w_plane, int32_t R, int32_t N, int32_t K,
                         int32_t num, int32_t epi, const float* bias, const float* post_slope, const float* gamma, const float* res,
                         const float* aux, int32_t ldr, int32_t nsplit, float* y, int32_t ldy, int32_t ycols, void* ya, int64_t ya_plane,
                         int32_t ldya, int32_t pcol0, const float* next_slope, void* stream);

/* The folded single-query attention of the CLS-only last layer (csrc/cls_tail.hip) with its value projection: for each of nseq sequences
 * (S fp32 rows of H at x + r * seq_stride, in elements) and its one query q[r][H] (fp32; q_log2 != 0, 3-term formats only: already scaled by
 * 1/sqrt(64) * log2(e)):
 *     ctx[r][64h + d] = sum_s softmax_s(q_h . K_h[s] / sqrt(64)) V[s][64h + d],   K, V = the key / value projections of LayerNorm(x; ln_w, ln_b)
 * evaluated WITHOUT forming K or V: scores against u = W_k,h^T q_h, a weighted sum of the normalised rows, then W_v of that sum.
 * wqkv: the packed [3H][H] query | key | value weight as 16-bit planes of format `num` (VTQ_NUM_*), bqkv fp32 [3H] (only the value part is read:
 * q . b_k is constant per head).  Caller workspace: u fp32 [nseq][H/64][H]; part fp32 [nseq][ceil(S / vtq_k_cls_fold_chunk_rows())][H/64][H + 2];
 * z: 16-bit planes [planes of an activation][ceil64(nseq)][H/64 * H], z_plane elements apart.  ctx: fp32 [nseq][H].  H = 768 | 1024.
 * A sequence's result depends on its own rows and on S only, never on nseq.
 * Extents: exactly the sizes above.  x: rows [0, S) of each sequence are read, the elements [S * H, seq_stride) behind them never
 * (seq_stride % 4 == 0).  u, part and z need no initial value; rows [0, nseq) of z are written, rows [nseq, ceil64(nseq)) are read by
 * the value projection and reach no output.  wqkv: rows [H, 3H) of every plane are read; ln_w, ln_b fp32 [H]; q fp32 [nseq][H]. */
int  vtq_k_cls_fold(const float* q, const void* wqkv, int64_t w_plane, const float* bqkv, const float* x, int64_t seq_stride,
                    const float* ln_w, const float* ln_b, int32_t nseq, int32_t S, int32_t H, int32_t num, int32_t q_log2,
                    float* u, float* part, void* z, int64_t z_plane, float* ctx, void* stream);
/* HOST-only: rows of a sequence per partial of vtq_k_cls_fold (a compile-time constant). */
int  vtq_k_cls_fold_chunk_rows(void);
/* vtq_k_cls_fold over nseq sequences of DIFFERENT lengths packed back to back, the table-driven form vtq_forward_varlen, vtq_forward_group and
 * the cached entries run: sequence j is the seq_len[j] >= 1 rows from row0[j] = sum_{i<j} seq_len[i] (seq_len: HOST int32[nseq], nseq <= 65535);
 * with R = the sum of all lengths and S_max = the largest:
 *   x     fp32 [R][H]: rows [row0[j], row0[j] + seq_len[j]) are read for sequence j and nothing else -- no row at or behind R, and no row of
 *         another sequence reaches sequence j's result.
 *   q     fp32 [nseq][H], one query per sequence.  wqkv, bqkv, ln_w, ln_b, q_log2, num: as vtq_k_cls_fold.
 *   u     fp32 [nseq][H/64][H];  part fp32 [nseq][ceil(S_max / vtq_k_cls_fold_chunk_rows())][H/64][H + 2]: a sequence writes and reads the
 *         chunks of its own length only, the others of its slot are not touched;  z, ctx: as vtq_k_cls_fold (exactly those sizes).
 * Row j of ctx has the bits vtq_k_cls_fold(nseq = 1, S = seq_len[j]) gives on that sequence's rows and query.  A test entry: it uploads its
 * row-offset and length tables to a temporary and waits for `stream` before returning. */
int  vtq_vl_cls_fold(const float* q, const void* wqkv, int64_t w_plane, const float* bqkv, const float* x, const float* ln_w, const float* ln_b,
                     int32_t nseq, const int32_t* seq_len, int32_t H, int32_t num, int32_t q_log2, float* u, float* part, void* z,
                     int64_t z_plane, float* ctx, void* stream);

/* The DiffNet head + quality predictor alone (quality_decoder -> q_predictor, vtamiq.py:114-117, channel_attention.py:13-86) with
 * the handle's loaded weights: d fp32 [HB][H] = diff_scale(cls_ref - cls_dist) -> q_out fp32 [HB] (HB >= 1; exactly these extents are read
 * and written: every intermediate lives in the handle's workspace). */
int  vtq_k_diffnet_head(vtq_handle h, const float* d, int32_t HB, float* q_out, void* stream);

/* ---- on-device image -> patch tensor; replaces the CPU loader's transform_img (data/utils.py:76-94) and the
 * gather / position / pyramid part of get_iqa_patches (data/patch_sampling.py:529-611) for GIVEN sample coordinates ---------- */
/* images uint8 [NI, H, W, 3] -> out fp32 [NI, 3, H, W] = ((x / 255) - mean[c]) / std[c]; flips: DEVICE int32 [NI][2] = (hflip, vflip)
 * or NULL; mean/std: HOST float[3]. */
int  vtq_k_image_normalize(const uint8_t* images, float* out, int32_t NI, int32_t H, int32_t W, const int32_t* flips,
                           const float* mean, const float* std_, void* stream);
/* torch.nn.AvgPool2d(2): in [NC, H, W] -> out [NC, H/2, W/2] (an odd last row / column is dropped; H, W >= 2). */
int  vtq_k_avgpool2(const float* in, float* out, int32_t NC, int32_t H, int32_t W, void* stream);
/* levels: HOST array of nlevels (<= 4) DEVICE pointers to [NI, 3, hs[l], ws[l]]; samples DEVICE int32 [NI, N, 2] (row, col at the
 * patch's own scale); scale_ids DEVICE int32 [NI, N] or NULL (all scale 0); patch_size P = 16 | 8.  Outputs: patches [NI, N, 3, P, P],
 * pos [NI, N, 2] = clamp((sample + P/2) / (dim - P/2), 0, 1 - 1e-6), scales [NI, N] (fp32-cast ids, may be NULL).
 * A sample must lie inside its level (0 <= row <= hs[l] - P, 0 <= col <= ws[l] - P: the kernel does not check; a corner patch reads the
 * level's last element and nothing behind it).  patch_size other than 16 | 8 and nlevels outside 1 .. 4 are refused. */
int  vtq_k_gather_patches(const float* const* levels, const int32_t* hs, const int32_t* ws, int32_t nlevels, const int32_t* samples,
                          const int32_t* scale_ids, float* patches, float* pos, float* scales, int32_t NI, int32_t N, int32_t patch_size,
                          void* stream);

/* ---- validation-loop reductions; fp64 like the reference's numpy arrays ------------------------------------ */
/* average_over_repeats (train.py:398-400): q fp32 [R, N] (repeat-major, as the concatenated passes of do_validation) ->
 * out fp64 [N] = mean over the R repeats, summed in repeat order from +0 (numpy's axis-0 reduction: a column of -0.0 alone gives +0.0).
 * Non-finite scores follow IEEE arithmetic as in numpy: a NaN, or +inf and -inf in one column, gives NaN; otherwise an infinity stays.
 * R, N >= 1. */
int  vtq_k_repeat_mean(const float* q, double* out, int32_t R, int32_t N, void* stream);
/* The fit-free part of compute_correlations (utils/misc/correlations.py:21-33) on two fp64 score vectors a, b [N]:
 *   work[0:N], work[N:2N]  = normalize_array(a), normalize_array(b) (image_tools.py:17-21; plain copies when normalize == 0)
 *   work[2N:3N], [3N:4N]   = their average-tie ranks
 *   counts[0] = 2 (concordant - discordant pairs), counts[1] = 2 (pairs tied in a), counts[2] = 2 (pairs tied in b)   (exact)
 *   out[0] = Spearman (Pearson of the ranks), out[1] = Pearson, out[2] = RMSE of the normalised vectors.
 * work: DEVICE fp64 [4N]; counts: DEVICE int64 [3]; out: DEVICE fp64 [3] (exactly; none needs an initial value).  N >= 2.  The host
 * finishes Kendall's tau-b from the counts.
 * Degenerate input follows numpy / scipy.stats, never a value that reads as a good model:
 *   - a NaN anywhere in a or b gives NaN for out[0], out[1] and out[2].  With normalize != 0 the vector's whole normalised copy is NaN
 *     (ndarray.min / max propagate), with normalize == 0 the NaN element alone; a NaN element has a NaN rank.  The pair kernel counts a NaN
 *     as tied with everything, so the counts stay finite: the caller reports Kendall as NaN when work[0:2N] holds a NaN.
 *   - a constant a or b gives NaN for out[0] and out[1] (scipy.stats.pearsonr's constant-input rule, also where the mean of N equal values
 *     rounds away from that value); out[2] stays finite; counts[1] or counts[2] equals N (N - 1), the "no tau" condition.
 *   - infinities behave as in numpy: they rank and count like any other value; inf - inf is NaN in the normalised copy (-inf with
 *     normalize != 0) and in Pearson's centring, so out[1] is NaN and out[2] is inf or NaN. */
int  vtq_k_rank_metrics(const double* a, const double* b, int32_t N, int32_t normalize, double* work, int64_t* counts, double* out,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VTAMIQ_HIP_H */
