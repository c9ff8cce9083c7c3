/*
 * vtamiq_hip_rollout.h -- the per-kernel entry point of the attention-rollout step (csrc/attention_rollout.hip), exported by libvtamiq_hip.so
 * beside the entries of vtamiq_hip.h, whose conventions apply (device pointers, asynchronous on `stream`, 0 = ok, vtq_last_error).  The
 * scoring entries that use the step are vtq_forward_rollout / vtq_forward_rollout_tokens in vtamiq_hip.h; this one exists for unit tests.
 * It has a header of its own because the per-kernel table of vtamiq_hip.h is pinned entry by entry by tests/test_gpu_footprint.py; the
 * footprint of this entry is pinned by tests/test_gpu_rollout.py.
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

#ifdef __cplusplus
}
#endif
#endif /* VTAMIQ_HIP_ROLLOUT_H */
