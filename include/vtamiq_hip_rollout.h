/*
 * vtamiq_hip_rollout.h -- the per-kernel entry points of the attention-rollout step (csrc/attention_rollout.hip), exported by libvtamiq_hip.so
 * beside the entries of vtamiq_hip.h, whose conventions apply (device pointers, asynchronous on `stream`, 0 = ok, vtq_last_error).  The
 * scoring entries that use the step are vtq_forward_rollout / vtq_forward_rollout_tokens in vtamiq_hip.h; these exist for unit tests.
 * They have a header of their own because the per-kernel table of vtamiq_hip.h is pinned entry by entry by tests/test_gpu_footprint.py; the
 * footprint of vtq_k_rollout_step is pinned by tests/test_gpu_rollout.py, that of vtq_vl_rollout_step by tests/test_gpu_rollout_entries.py.
 */
#ifndef VTAMIQ_HIP_ROLLOUT_H
#define VTAMIQ_HIP_ROLLOUT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One attention-rollout step on the qkv planes of vtq_k_attention (num = VTQ_NUM_* with 1 or 3 terms; q_log2 as vtq_k_attention_probs): with P[s][hd] the
 * probabilities vtq_k_attention_probs would store,
 *     r_out[s][j] = 1/2 r_in[s][j] + 1/(2 H/64) sum_hd sum_i r_in[s][i] P[s][hd][i][j]
 * without storing any of them.  r_in, r_out: fp32, exactly nseq * S floats each (distinct buffers); part: workspace fp32, exactly
 * nseq * (H / 64) * ceil(S / 128) * S floats, no initial value needed.  Reads only rows [s * S_pad, s * S_pad + S) of sequence s (qkv:
 * planes of nseq * S_pad rows suffice; the value columns are not read).  A sequence's result depends on its own rows and S only. */
int  vtq_k_rollout_step(const void* qkv, int64_t plane, const float* r_in, float* r_out, float* part, int32_t nseq, int32_t S, int32_t S_pad,
                        int32_t H, int32_t num, int32_t q_log2, void* stream);

/* The same step over nseq sequences of DIFFERENT lengths packed back to back, the layout vtq_forward_varlen leaves in the QKV planes (and
 * vtq_vl_attention reads): seq_len = HOST int32[nseq], every entry >= 1, nseq <= 65535; sequence j is the seq_len[j] rows from row0[j] = the
 * sum of the lengths before it, R = the sum of all of them, S_max the largest.
 *   r_in, r_out : fp32, exactly R floats each (distinct buffers), packed like the rows: sequence j's vector is the seq_len[j] floats at row0[j]
 *   part        : workspace fp32, exactly (H / 64) * ceil(S_max / 128) * R floats, no initial value needed
 *                 (part[(head * ceil(S_max / 128) + block) * R + row0[j] + key]; blocks >= ceil(seq_len[j] / 128) of a sequence are not touched)
 * Reads only the rows [row0[j], row0[j] + seq_len[j]) of sequence j -- planes of R rows suffice, the value columns are not read -- and writes
 * nothing outside a sequence's own seq_len[j] outputs.  Sequence j's r_out has the bits vtq_k_rollout_step gives for that sequence alone
 * (nseq = 1, S = S_pad = seq_len[j]) on the same rows: the two kernels share the step's body, and every summation order is a function of
 * seq_len[j] alone.  The block table (vtq_vl_attention_blocks) is built and uploaded inside the call, which therefore synchronises `stream`. */
int  vtq_vl_rollout_step(const void* qkv, int64_t plane, const float* r_in, float* r_out, float* part, int32_t nseq, const int32_t* seq_len,
                         int32_t H, int32_t num, int32_t q_log2, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VTAMIQ_HIP_ROLLOUT_H */
