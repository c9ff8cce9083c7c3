// libvtamiq_hip.so: C ABI (include/vtamiq_hip.h) around the gfx950 kernels.
//
// One engine = one VTAMIQ model instance on one GPU: packed weights (16-bit hi[/lo] planes for the ViT GEMMs, fp32 for
// everything else), a workspace sized for the largest (B, N) seen, and the launch sequence of VTAMIQ.forward
// (modules/vtamiq/vtamiq.py:94-119) with both images of a pair batched as 2B sequences through ONE encoder pass
// (the reference runs two serial passes with the same weights, vtamiq.py:100-101).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <climits>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/vtamiq_hip.h"
#include "../../include/vtamiq_hip_fp8.h"
#include "../../include/vtamiq_hip_rollout.h"
#include "../../include/vtamiq_hip_images.h"
#include "../../include/vtamiq_hip_tensors.h"
#include "../../include/vtamiq_hip_sampler.h"
#include "../../include/vtamiq_hip_weighted_sampler.h"
#include "kernels.h"

using namespace vtq;

namespace {

thread_local std::string g_err;

int fail(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return 1;
}

#define HIP_TRY(expr)                                                                           \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) return fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

// fp8 mode: per-tensor power-of-two activation scales (value * scale is rounded to e4m3, |.| clamped to 448), one per
// quantisation point: the packed patches, and per layer the LayerNorm-1 output, the attention context, the LayerNorm-2 output and
// the GELU output.  They start at the round-2 constants below (oracle/fp8_oracle.py STATIC carries the same) and are replaced by
// CALIBRATED ones: the first forward of an engine (or vtq_fp8_calibrate on a batch of the caller's choice) measures max |value| at
// every point on that batch -- each producing kernel reports it (kernels.h Fp8Obs) and is run again once its scale is chosen, so
// everything downstream already sees the final operands -- and takes the largest power of two that maps it to <= 224 (a factor two
// of headroom for other batches; e4m3 is a floating format, so headroom costs no precision until values underflow 2^-9).
// vtq_config.options & VTQ_OPT_FP8_STATIC_SCALES keeps the constants.  A value that still exceeds 448 after scaling is clamped and raises bit 2 of the
// error word (vtq_input_errors).
constexpr float kSPatch = 256.0f, kSLn = 8.0f, kSAtt = 16.0f, kSGelu = 4.0f;
[[maybe_unused]] constexpr float kFp8Target = 224.0f;

// Softmax scale of MultiHeadSelfAttention (transformer.py:158-160: scores / sqrt(head_dim), head_dim = 64) times log2(e): with the
// 3-term attention the engine folds it into the query projection at weight ingestion, so that scores arrive in log2 units and the
// kernels' exponent is exp2(s - max) -- a subtraction that is exact for the row maximum at any magnitude (attention.hip prescale_q).
constexpr float kQLog2Scale = 0.125f * 1.4426950408889634f;

struct Slot {
    void* dst = nullptr;      // destination (fp32 copy) or bf16 hi plane (split)
    int64_t numel = 0;
    bool split = false;       // true: pack to 16-bit planes (engine->f16, engine->wpl), or to e4m3 rows + per-row scales (fp8 mode)
    int64_t plane = 0;        // elements between hi and lo plane
    float* scale = nullptr;   // fp8 mode: destination of the rows' inverse scales
    int64_t K = 0;            // row length of a split tensor
    int64_t Kp = 0;           // row pitch of its packed planes (> K: zero-padded to the GEMM's K tile; 0 = K)
    float mul = 1.0f;         // the tensor is multiplied by this on ingestion (query projection: kQLog2Scale)
    bool ignore = false;      // accepted and dropped: a parameter the forward never reads (adapter pairs other than pair 0)
    bool loaded = false;
};

// One linear layer y = x W^T + b as the GEMM and skinny kernels read it: weight planes [N][K] (16-bit, `plane` elements from hi to
// lo; fp8 mode: e4m3 rows + per-output-channel inverse scales) and an fp32 bias.  K is the row pitch of the packed planes, i.e. the
// kernel's K: a tensor with shorter rows is zero-padded to it.
struct Lin { void* w = nullptr; int64_t plane = 0; float* wscale = nullptr; float* b = nullptr; int N = 0, K = 0; };
// rows [row0, row0 + n) of l as a layer of its own (esz: bytes per weight element)
Lin lin_rows(const Lin& l, int64_t row0, int64_t n, int esz = 2) {
    return Lin{(char*)l.w + row0 * l.K * esz, l.plane, l.wscale ? l.wscale + row0 : nullptr, l.b + row0, (int)n, l.K};
}
// Activation planes [rows][ld] of lnbuf / big / the tail and head buffers (`plane` elements from hi to lo)
struct View { void* p = nullptr; int64_t plane = 0; int ld = 0; };

// out = A W^T + b over M rows: the operands of one launch_gemm; epilogue-specific fields (gamma, x, row_map ...) are the caller's
GemmArgs gemm_args(View a, const Lin& l, int M, View out = View{}, float ascale_inv = 0.0f) {
    GemmArgs g{};
    g.A = a.p; g.a_plane = a.plane; g.lda = a.ld; g.W = l.w; g.w_plane = l.plane; g.M = M; g.N = l.N; g.K = l.K; g.bias = l.b;
    g.out = out.p; g.o_plane = out.plane; g.ldo = out.ld; g.wscale = l.wscale; g.ascale_inv = ascale_inv;
    return g;
}
// the same for one skinny stage on R rows (CLS tail, DiffNet head); ya_planes: planes of its 16-bit output, if it writes one
SkinnyArgs skinny_args(View x, const Lin& l, int R, int ya_planes) {
    SkinnyArgs a{};
    a.xa = x.p; a.xa_plane = x.plane; a.ldx = x.ld; a.W = l.w; a.w_plane = l.plane; a.R = R; a.N = l.N; a.K = l.K; a.bias = l.b;
    a.ya_planes = ya_planes;
    return a;
}

struct Layer {
    Lin qkv, out, fc1, fc2;                    // qkv: query, key, value rows stacked ([3H][H])
    float *ln1w = nullptr, *ln1b = nullptr, *ln2w = nullptr, *ln2b = nullptr, *g1 = nullptr, *g2 = nullptr;
    // Adapter pair 0 (transformer.py:177-194, 260-269): site 0 after attention, site 1 after the MLP.  down: [Hq_pad, H] planes
    // (rows >= H/4 zero), up: [H, Hq_pad] planes (K zero-padded); Hq_pad = H/4 rounded up to the GEMM tile (256)
    Lin ad_dn[2], ad_up[2];
};
// The DiffNet head's linear stages are Lin too: fp16 hi/lo planes [2][ceil16(N)][K] (K padded to the skinny kernel's 32-deep k-step
// with zeros), packed by pack_head.  The head always runs the 3-term fp16 form, whatever the encoder's precision.
struct Rcab { float *slope, *w, *b, *wd, *bd, *wu, *bu, *wcat, *bcat; Lin cat, up; };   // wcat/bcat: [Wc ; Wd Wc], folded at load time
struct Rg { std::vector<Rcab> rcabs; float *w, *b; Lin tail; };

}  // namespace

struct vtq_engine {
    vtq_config cfg{};
    Num lin{0, 1}, att{0, 1};          // operand format of the linear layers / of attention (QK^T, PV)
    int f16 = 0, apl = 1, wpl = 1;     // element type of every plane; planes per activation / per weight tensor
    int dbg_stop = -1;                 // tests: leave the encoder after stage layer * 7 + k (vtq_debug_stop_after), -1 = never
    bool fp8 = false;                  // linear layers on e4m3 operands (MX-scaled MFMA, unit block scales): VTQ_PREC_FP8
    float s_patch = kSPatch;           //   activation scales (see kSPatch ...): patches, then per layer {LN1, attention, LN2, GELU}
    std::vector<float> s_ln1, s_att, s_ln2, s_gelu;
    bool fp8_static = false, fp8_calibrated = false;
    bool fp8_installed = false;        //   the current scales came from vtq_fp8_set_scales: a weight reload keeps them
    float* amax_slot = nullptr;        //   device word the producers report max |value| into during a calibration forward
    int64_t PDp = 0;                   // patch_dim rounded up to the GEMM's K granule (row pitch of the packed patches / weight)
    int64_t Hqp = 0;                   // adapters: H / 4 rounded up to the GEMM tile (N of the down projection, K of the up projection)
    int H = 0, Mdim = 0, T = 0;
    std::vector<void*> allocs;
    std::unordered_map<std::string, Slot> slots;
    // ViT
    Lin patch;                         // patch embedding: [H][PDp]
    float *cls = nullptr, *extra = nullptr, *pos_table = nullptr, *scale_table = nullptr, *encw = nullptr, *encb = nullptr;
    std::vector<Layer> layers;
    // head
    float* diff_gamma = nullptr;
    std::vector<Rg> rgs;
    float *qdw = nullptr, *qdb = nullptr, *p1w = nullptr, *p1b = nullptr, *p2a = nullptr, *p4w = nullptr, *p4b = nullptr;
    Lin qd, p1, p4;
    // workspace
    int capB = 0, capN = 0;
    float* x = nullptr;
    void *lnbuf = nullptr, *big = nullptr;
    int64_t ln_plane = 0, big_plane = 0;
    int *pidx = nullptr, *sidx = nullptr, *row_map = nullptr;
    float* hb[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    float* hhid = nullptr;
    int r_alloc = 0;                     // rows of the skinny-stage plane buffers (multiple of 64)
    void *hp[2] = {nullptr, nullptr}, *ht = nullptr, *hq = nullptr;   // head planes (fp16 hi/lo): [r_alloc][H] x2, [r_alloc][hidp], [r_alloc][H/4]
    int64_t hp_plane = 0, ht_plane = 0, hq_plane = 0;
    int hidp = 0;
    void *tl = nullptr, *th = nullptr;   // CLS-tail planes (encoder format): [r_alloc][H], [r_alloc][M]
    int64_t tl_plane = 0, th_plane = 0;
    float *xcls = nullptr, *lncls = nullptr, *qcls = nullptr;   // CLS-only last layer (fp32 rows)
    float *fold_u = nullptr, *fold_part = nullptr;              //   folded attention (cls_tail.hip): W_k^T q per (sequence, head); chunk partials
    void* fold_z = nullptr;                                      //   its output planes (encoder format): [r_alloc][H / 64 * H]
    int64_t fold_z_plane = 0;
    // One call's device table (upload_table; its sections: Table below).  Built on the host in a pinned image of this engine's own and
    // uploaded on the call's stream ahead of the first launch.  vl_uploaded: recorded behind the upload, waited for before the next call
    // rewrites the image.  Per engine: nothing of this is shared between handles.
    int* vl_tab = nullptr;               //   device (workspace)
    int* vl_host = nullptr;              //   pinned host image
    size_t vl_host_ints = 0;
    hipEvent_t vl_uploaded = nullptr;
    bool cls_prune = true;
    bool fuse_ln = false;                // VTQ_OPT_FUSED_LAYERNORM: residual GEMMs carry the next LayerNorm in their epilogue (gemm_rowln.hip)
    int32_t* err_host = nullptr;         // pinned landing word of vtq_input_errors (a pageable destination goes through the runtime's staging path)
    int* err_flag = nullptr;             // device word (vtq_input_errors): bit 0 = a position outside [0, 1) was clamped, bit 1 = non-finite CLS difference
    std::vector<void*> ws_allocs;
    float* trace = nullptr;
    // vtq_forward_rollout: the workspace only such a call reserves (rollout_workspace): one QKV buffer per layer, in which its Q / K planes
    // survive the forward, the row vector (ping-pong), the step's partials
    int ro_capB = 0, ro_capN = 0;
    std::vector<void*> ro_qkv;                  // one slot per layer (vtq_create)
    int64_t ro_plane = 0;
    float *ro_r[2] = {nullptr, nullptr}, *ro_part = nullptr;
    std::vector<void*> ro_allocs;
    int iqa_token = 0;                          // vtamiq.py:57, 107-108: the token row the head consumes (0 = CLS, 1 .. = register tokens)
    // profiling
    uint32_t prof_mask = 0;
    struct Ev { hipEvent_t a, b; int cls; };
    std::vector<Ev> ev_used;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_free;
};

namespace {

int dev_alloc(vtq_engine* e, void** p, size_t bytes) {
    HIP_TRY(hipMalloc(p, bytes ? bytes : 16));
    e->allocs.push_back(*p);
    return 0;
}

int add_f32(vtq_engine* e, const std::string& name, float** p, int64_t numel) {
    if (dev_alloc(e, (void**)p, numel * sizeof(float))) return 1;
    Slot s; s.dst = *p; s.numel = numel;
    e->slots[name] = s;
    return 0;
}

// Allocates one linear layer of operand format `num`: [rows][K] weight planes (rows: N, or more where the kernel reads whole tiles),
// an fp32 bias of its own unless `bias` names one, and for e4m3 weights the inverse scales.  zero: the padding no load slot covers
// is read by the kernels and must be zero.
int add_lin(vtq_engine* e, Lin& l, Num num, int64_t N, int64_t K, bool zero = false, float* bias = nullptr, int64_t rows = 0) {
    if (rows == 0) rows = N;
    l.N = (int)N; l.K = (int)K; l.plane = rows * K; l.b = bias;
    const size_t wbytes = (size_t)l.plane * 2 * num.wpl();
    if (dev_alloc(e, &l.w, wbytes) || (!bias && dev_alloc(e, (void**)&l.b, rows * sizeof(float))) ||
        (num.f16 == 2 && dev_alloc(e, (void**)&l.wscale, rows * sizeof(float))))
        return 1;
    if (zero) {
        HIP_TRY(hipMemset(l.w, 0, wbytes));
        if (!bias) HIP_TRY(hipMemset(l.b, 0, rows * sizeof(float)));
    }
    return 0;
}

// load slots `name`.weight ([rows, K] fp32; K < l.K: zero-padded to the planes' row pitch) and `name`.bias for rows [row0, row0 + rows) of l
void lin_slots(vtq_engine* e, const Lin& l, const std::string& name, int64_t rows, int64_t K, int64_t row0 = 0) {
    const Lin r = lin_rows(l, row0, rows, e->fp8 ? 1 : 2);
    Slot w; w.dst = r.w; w.numel = rows * K; w.split = true; w.plane = r.plane; w.scale = r.wscale; w.K = K; w.Kp = r.K;
    e->slots[name + ".weight"] = w;
    Slot b; b.dst = r.b; b.numel = rows;
    e->slots[name + ".bias"] = b;
}

int build(vtq_engine* e) {
    const vtq_config& c = e->cfg;
    const int64_t H = c.hidden_size, M = c.mlp_dim, PD = c.patch_dim;
    const std::string emb = "transformer.embeddings.";
    if (add_f32(e, emb + "cls_token", &e->cls, H)) return 1;
    if (c.num_extra_tokens > 0 && add_f32(e, emb + "extra_tokens", &e->extra, (int64_t)c.num_extra_tokens * H)) return 1;
    // the patch-embedding GEMM runs on K padded to 256 (two K tiles of every operand format): 768 as is, ViT-B/8's 192 -> 256
    e->PDp = round_up(PD, 256);
    e->Hqp = round_up(H / 4, 256);
    if (add_lin(e, e->patch, e->lin, H, e->PDp)) return 1;
    lin_slots(e, e->patch, emb + "patch_embeddings", H, PD);
    if (add_f32(e, emb + "positional_embeddings.positional_embeddings", &e->pos_table, ((int64_t)c.pos_grid * c.pos_grid + 1) * H))
        return 1;
    if (c.num_scales > 1 && add_f32(e, emb + "scale_embeddings.scale_embeddings", &e->scale_table, ((int64_t)c.num_scales + 1) * H))
        return 1;
    const std::string enc = "transformer.encoder.";
    if (add_f32(e, enc + "encoder_norm.weight", &e->encw, H) || add_f32(e, enc + "encoder_norm.bias", &e->encb, H)) return 1;
    e->layers.resize(c.num_layers);
    for (int i = 0; i < c.num_layers; ++i) {
        Layer& L = e->layers[i];
        const std::string p = enc + "layers." + std::to_string(i) + ".";
        if (add_lin(e, L.qkv, e->lin, 3 * H, H) || add_lin(e, L.out, e->lin, H, H) || add_lin(e, L.fc1, e->lin, M, H) ||
            add_lin(e, L.fc2, e->lin, H, M))
            return 1;
        const char* qkvn[3] = {"query", "key", "value"};
        for (int j = 0; j < 3; ++j) lin_slots(e, L.qkv, p + "attn." + qkvn[j], H, H, j * H);
        if (e->att.terms == 3) {       // 3-term attention takes Q in log2 units: (x W_q + b_q) * kQLog2Scale, folded into W_q and b_q
            e->slots[p + "attn.query.weight"].mul = kQLog2Scale;
            e->slots[p + "attn.query.bias"].mul = kQLog2Scale;
        }
        lin_slots(e, L.out, p + "attn.out", H, H);
        lin_slots(e, L.fc1, p + "ffn.fc1", M, H);
        lin_slots(e, L.fc2, p + "ffn.fc2", H, M);
        if (add_f32(e, p + "attention_norm.weight", &L.ln1w, H) || add_f32(e, p + "attention_norm.bias", &L.ln1b, H) ||
            add_f32(e, p + "ffn_norm.weight", &L.ln2w, H) || add_f32(e, p + "ffn_norm.bias", &L.ln2b, H))
            return 1;
        if (c.use_layer_scale && (add_f32(e, p + "ls1.gamma", &L.g1, H) || add_f32(e, p + "ls2.gamma", &L.g2, H))) return 1;
        if (c.num_adapters > 0) {
            const int64_t Hq = H / 4, Hqp = e->Hqp;
            for (int site = 0; site < 2; ++site) {
                const std::string q = p + "adapter" + std::to_string(site + 1) + ".adapter.";
                // down: rows >= Hq keep zero weights and a zero bias -> gelu(0) = 0
                if (add_lin(e, L.ad_dn[site], e->lin, Hqp, H, true) || add_lin(e, L.ad_up[site], e->lin, H, Hqp)) return 1;
                lin_slots(e, L.ad_dn[site], q + "0", Hq, H);
                lin_slots(e, L.ad_up[site], q + "2", H, Hq);
            }
            for (int a = 3; a <= 2 * c.num_adapters; ++a) {          // pairs >= 1 exist in the state_dict; the forward never reads them
                const std::string q = p + "adapter" + std::to_string(a) + ".adapter.";
                const int64_t n[4] = {Hq * H, Hq, H * Hq, H};
                const char* nm[4] = {"0.weight", "0.bias", "2.weight", "2.bias"};
                for (int k = 0; k < 4; ++k) { Slot sg; sg.numel = n[k]; sg.ignore = true; e->slots[q + nm[k]] = sg; }
            }
        }
    }
    if (c.diff_scale && add_f32(e, "diff_scale.gamma", &e->diff_gamma, H)) return 1;
    if (c.calibrate) {
        const int64_t hid = c.ca_hidden;
        e->rgs.resize(c.num_rgs);
        for (int g = 0; g < c.num_rgs; ++g) {
            Rg& R = e->rgs[g];
            R.rcabs.resize(c.num_rcabs);
            for (int k = 0; k < c.num_rcabs; ++k) {
                Rcab& r = R.rcabs[k];
                const std::string p = "quality_decoder." + std::to_string(g) + ".body." + std::to_string(k) + ".body.";
                if (add_f32(e, p + "1.weight", &r.slope, 1) || add_f32(e, p + "2.weight", &r.w, H * H) ||
                    add_f32(e, p + "2.bias", &r.b, H) || add_f32(e, p + "4.conv_du.1.weight", &r.wd, hid * H) ||
                    add_f32(e, p + "4.conv_du.1.bias", &r.bd, hid) || add_f32(e, p + "4.conv_du.4.weight", &r.wu, H * hid) ||
                    add_f32(e, p + "4.conv_du.4.bias", &r.bu, H))
                    return 1;
                if (dev_alloc(e, (void**)&r.wcat, (size_t)(H + hid) * H * 4) || dev_alloc(e, (void**)&r.bcat, (size_t)(H + hid) * 4)) return 1;
            }
            const std::string p = "quality_decoder." + std::to_string(g) + ".body." + std::to_string(c.num_rcabs) + ".";
            if (add_f32(e, p + "weight", &R.w, H * H) || add_f32(e, p + "bias", &R.b, H)) return 1;
        }
        const std::string p = "quality_decoder." + std::to_string(c.num_rgs) + ".";
        if (add_f32(e, p + "weight", &e->qdw, H * H) || add_f32(e, p + "bias", &e->qdb, H)) return 1;
    }
    if (add_f32(e, "q_predictor.1.weight", &e->p1w, (H / 4) * H) || add_f32(e, "q_predictor.1.bias", &e->p1b, H / 4) ||
        add_f32(e, "q_predictor.2.weight", &e->p2a, 1) || add_f32(e, "q_predictor.4.weight", &e->p4w, H / 4) ||
        add_f32(e, "q_predictor.4.bias", &e->p4b, 1))
        return 1;
    // fp16 hi/lo planes of every head matrix (filled by pack_head after each weight load)
    auto head_lin = [&](Lin& L, int N, int K, float* bias) { return add_lin(e, L, Num{1, 3}, N, round_up(K, 32), true, bias, round_up(N, 16)); };
    if (c.calibrate) {
        for (auto& R : e->rgs) {
            for (auto& r : R.rcabs)
                if (head_lin(r.cat, (int)H + c.ca_hidden, (int)H, r.bcat) || head_lin(r.up, (int)H, c.ca_hidden, r.bu)) return 1;
            if (head_lin(R.tail, (int)H, (int)H, R.b)) return 1;
        }
        if (head_lin(e->qd, (int)H, (int)H, e->qdb)) return 1;
    }
    if (head_lin(e->p1, (int)H / 4, (int)H, e->p1b) || head_lin(e->p4, 1, (int)H / 4, e->p4b)) return 1;
    e->hidp = (int)round_up(c.ca_hidden > 0 ? c.ca_hidden : 32, 32);
    return 0;
}

// fp32 matrices of the head -> the fp16 planes the skinny kernel streams (after the CA fold); enqueued on s
int pack_head(vtq_engine* e, hipStream_t s) {
    auto pack = [&](const Lin& L, const float* W, int K) {       // K: row length of W (L.K is its 32-padded pitch)
        HIP_TRY(launch_rows_to_planes(W, K, nullptr, L.w, L.plane, L.K, L.N, K, 1, 2, s));
        return 0;
    };
    const int H = e->H, hid = e->cfg.ca_hidden;
    for (auto& R : e->rgs) {
        for (auto& r : R.rcabs) {
            HIP_TRY(launch_fold_ca(r.w, r.b, r.wd, r.bd, r.wcat, r.bcat, H, hid, s));
            if (pack(r.cat, r.wcat, H) || pack(r.up, r.wu, hid)) return 1;
        }
        if (pack(R.tail, R.w, H)) return 1;
    }
    if (e->cfg.calibrate && pack(e->qd, e->qdw, H)) return 1;
    return pack(e->p1, e->p1w, H) || pack(e->p4, e->p4w, H / 4);
}

struct Geometry {
    int S, S_pad, nseq;          // S_pad: row pitch of a sequence (= S: sequences are packed back to back)
    int64_t M_pad, P_pad, rows_alloc;
    int64_t R_pad;               // rows of the skinny-stage plane buffers (CLS tail, head): one per sequence, padded to the kernel's 64
    SeqMap sm;
};

// nseq sequences of N patches each -- any count: 2B or 3B for pairs and triplets, B single images, G + M for vtq_forward_group
Geometry geometry_seq(const vtq_engine* e, int nseq, int N) {
    Geometry g;
    g.S = N + e->T;
    // No per-sequence padding: attention masks keys >= S (its last 64-key tile and last 128-query block run into the next
    // sequence's rows, or into the tail / the 128 slack rows: finite values, never stored), every other kernel is
    // row-independent.  Only the whole batch is padded, to the GEMM tile height.
    g.S_pad = g.S;
    g.nseq = nseq;
    g.M_pad = round_up((int64_t)g.nseq * g.S_pad, 256);
    g.P_pad = round_up((int64_t)nseq * N, 256);
    // +128: attention over-read slack behind the last sequence.  vtq_k_attention's contract (include/vtamiq_hip.h) is ceil128(S_pad) - S_pad
    // <= 127 rows behind row nseq * S_pad <= M_pad, pinned by tests/test_gpu_footprint.py test_attention with exactly that many rows; 128 is
    // that bound rounded to the GEMM half tile, and the length of the memset in forward()
    g.rows_alloc = (g.M_pad > g.P_pad ? g.M_pad : g.P_pad) + 128;
    g.R_pad = round_up(g.nseq, 64);
    g.sm = SeqMap{g.S_pad, g.nseq, (int)(g.M_pad - (int64_t)g.nseq * g.S_pad)};
    return g;
}
// the capacity form: B sequence pairs of N patches
Geometry geometry(const vtq_engine* e, int B, int N) { return geometry_seq(e, 2 * B, N); }
// The variable-length entries: nseq sequences of sumN patches in all (every image counted), at most maxN in one.  Sequences packed back to
// back at their own length, so the row counts come from the sum; S is the largest sequence (the chunk pitch of the CLS fold's partials),
// and the map describes the whole batch as ONE run of rows, which is what the pad-row clear needs to know -- every other kernel addresses
// by the call's tables (VarLen)
Geometry geometry_varlen(const vtq_engine* e, int nseq, int64_t sumN, int maxN) {
    const int64_t rows = sumN + (int64_t)nseq * e->T;
    Geometry g;
    g.S = g.S_pad = maxN + e->T;
    g.nseq = nseq;
    g.M_pad = round_up(rows, 256);
    g.P_pad = round_up(sumN, 256);
    g.rows_alloc = (g.M_pad > g.P_pad ? g.M_pad : g.P_pad) + 128;
    g.R_pad = round_up(g.nseq, 64);
    g.sm = SeqMap{(int)rows, 1, (int)(g.M_pad - rows)};
    return g;
}

// THE layout of one call's device table (e->vl_tab), in ints.  A variable-length call of nseq sequences, M of them scored through ref_index
// (0: pairs, or vtq_encode_reference_varlen):
//     [0, nseq]          row offsets: sequence j is the rows [row0[j], row0[j + 1]) of the activation buffers
//     [len, len + nseq)  lengths S_j
//     [ref, ref + M)     ref_index
//     [blk, ...)         the attention block table, 4 ints per workgroup (attention_varlen.hip); the ints between ref + M and blk are zero
// There is no patch-row prefix: embed_index_kernel derives it from the row offsets.  A uniform group / cached call holds ref_index alone,
// at 0.  blk does not depend on M, so the table of any call of nseq sequences of at most S rows fits varlen_table_ints(nseq, S, H).
struct Table {
    int len, ref, blk;
    explicit Table(int nseq) : len(nseq + 1), ref(2 * nseq + 1), blk((int)round_up(3 * (int64_t)nseq + 4, 4)) {}      // ref + M <= 3 nseq + 1 <= blk
};
// upper bound in ints: blk, then 4 per attention workgroup -- sum_j ceil(S_j / 128) <= nseq * ceil(S / 128) query blocks per head
int64_t varlen_table_ints(int64_t nseq, int64_t S, int H) { return Table((int)nseq).blk + 4 * nseq * ((S + 127) / 128) * (H / 64); }

// One workspace buffer: the engine member it fills, its `planes` planes of `elems` elements of `esz` bytes (the plane stride goes
// to *stride where the engine keeps one), and whether reserve() zero-fills it.
struct WsBuf { void** ptr; int64_t* stride; int64_t elems; int esz, planes; bool zero; };

// THE description of the workspace for a capacity of B sequence pairs (2B sequences) of N patches: reserve() allocates it,
// vtq_workspace_bytes sums it.  Zero-filled are the buffers of which a kernel reads more than a forward writes: padded rows of x /
// lnbuf / big are computed on (never consumed) and must not breed NaNs; rows >= R and the K-padding columns of the skinny stages'
// planes are read by their MFMAs.
std::vector<WsBuf> workspace(vtq_engine* e, int B, int N) {
    const Geometry g = geometry(e, B, N);
    const int64_t H = e->H, Md = e->Mdim, Wmax = (3 * H > Md ? 3 * H : Md), rows = g.rows_alloc, R = g.R_pad;
    const int apl = e->apl;
    const int64_t nh = H / 64, chunks = (g.S + cls_fold_chunk_rows() - 1) / cls_fold_chunk_rows();
    std::vector<WsBuf> w = {
        {(void**)&e->x, nullptr, rows * H, 4, 1, true},                       // residual stream fp32
        {&e->lnbuf, &e->ln_plane, rows * H, 2, apl, true},                    // LayerNorm / attention output planes
        {&e->big, &e->big_plane, rows * Wmax, 2, apl, true},                  // qkv | mlp hidden | packed patches planes
        {(void**)&e->pidx, nullptr, g.P_pad, 4, 1, false},                    // pos / scale indices, row map
        {(void**)&e->sidx, nullptr, g.P_pad, 4, 1, false},
        {(void**)&e->row_map, nullptr, g.P_pad, 4, 1, false},
        {(void**)&e->hhid, nullptr, g.nseq * H, 4, 1, false},                 // head fp32 rows (pairwise: 2 scores per item)
        {(void**)&e->xcls, nullptr, g.nseq * H, 4, 1, false},                 // CLS-only last layer (fp32 rows)
        {(void**)&e->lncls, nullptr, g.nseq * H, 4, 1, false},
        {(void**)&e->qcls, nullptr, g.nseq * H, 4, 1, false},
        {&e->hp[0], &e->hp_plane, R * H, 2, 2, true},                         // head planes (fp16 hi/lo)
        {&e->hp[1], &e->hp_plane, R * H, 2, 2, true},
        {&e->ht, &e->ht_plane, R * e->hidp, 2, 2, true},
        {&e->hq, &e->hq_plane, R * (H / 4), 2, 2, true},
        {&e->tl, &e->tl_plane, R * H, 2, apl, true},                          // CLS-tail planes (encoder format)
        {&e->th, &e->th_plane, R * Md, 2, apl, true},
        {(void**)&e->fold_u, nullptr, g.nseq * nh * H, 4, 1, false},          // folded attention of the CLS-only last layer
        {(void**)&e->fold_part, nullptr, g.nseq * chunks * nh * (H + 2), 4, 1, false},
        {&e->fold_z, &e->fold_z_plane, R * nh * H, 2, apl, true},
    };
    for (float*& hb : e->hb) w.push_back({(void**)&hb, nullptr, g.nseq * H, 4, 1, false});   // head ping-pong rows
    w.push_back({(void**)&e->vl_tab, nullptr, varlen_table_ints(g.nseq, g.S, (int)H), 4, 1, false});   // one call's device table (Table)
    return w;
}

// vtq_forward_rollout's extra workspace (include/vtamiq_hip.h), held beside workspace() and reserved by such a call only: reserve_rollout()
// allocates it, vtq_rollout_workspace_bytes sums it.  One QKV buffer per layer, zero-filled as `big` is.  The last layer's too: the CLS
// tail never forms K, and its folded scores (fp32 rows against W_k^T q) are not the ones forward_vit reports -- they differ from them by
// the operand rounding of the mode, 2e-2 in bf16 on peaked attention -- so a rollout call projects the last layer's Q and K as well
// (run_encoder), and every layer's row comes from the same step kernel.
std::vector<WsBuf> rollout_workspace(vtq_engine* e, int B, int N) {
    const Geometry g = geometry(e, B, N);
    const int64_t r = (int64_t)g.nseq * g.S;
    std::vector<WsBuf> w;
    for (void*& q : e->ro_qkv) w.push_back({&q, &e->ro_plane, g.rows_alloc * 3 * e->H, 2, e->apl, true});
    w.push_back({(void**)&e->ro_r[0], nullptr, r, 4, 1, false});                              // the row vector (ping-pong)
    w.push_back({(void**)&e->ro_r[1], nullptr, r, 4, 1, false});
    w.push_back({(void**)&e->ro_part, nullptr, r * (e->H / 64) * ((g.S + 127) / 128), 4, 1, false});   // the step's partials
    return w;
}

size_t ws_bytes(const std::vector<WsBuf>& w) {
    size_t bytes = 0;
    for (const WsBuf& b : w) bytes += (size_t)b.elems * b.esz * b.planes;
    return bytes;
}

// Grows one of the two workspaces to the largest (B, N) seen: everything of it freed and allocated again.  The capacity is zero while
// that goes on, so a call behind a failed allocation allocates again.
int grow(vtq_engine* e, std::vector<WsBuf> (*list)(vtq_engine*, int, int), std::vector<void*>& owned, int& capB, int& capN, int B, int N) {
    if (B <= capB && N <= capN) return 0;
    const int nB = B > capB ? B : capB, nN = N > capN ? N : capN;
    HIP_TRY(hipDeviceSynchronize());
    for (void* p : owned) (void)hipFree(p);
    owned.clear();
    capB = capN = 0;
    const std::vector<WsBuf> bufs = list(e, nB, nN);
    for (const WsBuf& b : bufs) *b.ptr = nullptr;
    for (const WsBuf& b : bufs) {
        const size_t bytes = (size_t)b.elems * b.esz * b.planes;
        HIP_TRY(hipMalloc(b.ptr, bytes ? bytes : 16));
        owned.push_back(*b.ptr);
        if (b.stride) *b.stride = b.elems;
        if (b.zero) HIP_TRY(hipMemset(*b.ptr, 0, bytes));
    }
    HIP_TRY(hipDeviceSynchronize());
    capB = nB;
    capN = nN;
    return 0;
}

int reserve(vtq_engine* e, int B, int N) {
    if (grow(e, workspace, e->ws_allocs, e->capB, e->capN, B, N)) return 1;
    e->r_alloc = (int)geometry(e, e->capB, e->capN).R_pad;
    return 0;
}
int reserve_rollout(vtq_engine* e, int B, int N) { return grow(e, rollout_workspace, e->ro_allocs, e->ro_capB, e->ro_capN, B, N); }

struct Prof {
    vtq_engine* e; hipStream_t s; int cls; bool on; hipEvent_t a, b;
    Prof(vtq_engine* e_, hipStream_t s_, int cls_) : e(e_), s(s_), cls(cls_), on((e_->prof_mask >> cls_) & 1u) {
        if (!on) return;
        if (!e->ev_free.empty()) { a = e->ev_free.back().first; b = e->ev_free.back().second; e->ev_free.pop_back(); }
        else if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { on = false; return; }
        (void)hipEventRecord(a, s);
    }
    ~Prof() {
        if (!on) return;
        (void)hipEventRecord(b, s);
        e->ev_used.push_back({a, b, cls});
    }
};


// largest power of two s with m * s <= kFp8Target (exact: frexp, no log); 0 / non-finite m: keep `keep`
float fp8_pick_scale(float m, float keep) {
    if (!(m > 0.0f) || !std::isfinite(m)) return keep;
    int ex = 0;
    const float f = frexpf(m, &ex);                      // m = f * 2^ex, f in [0.5, 1);  224 = 0.875 * 2^8
    return ldexpf(1.0f, (f <= 0.875f ? 8 : 7) - ex);
}

// The one-to-many forms of a call (include/vtamiq_hip.h): which sequences it encodes and where the head's reference rows come from.
//   REF_GROUP   G references + B distorted images in one batch (nimg = 2), distorted image m scored against reference ref_index[m]
//   REF_ENCODE  B single reference images (nimg = 1): the consumed token's residual row of each goes to the caller's `rows`, no head
//   REF_CACHED  B single distorted images (nimg = 1) against the caller's G cached `rows`, through ref_index
enum { REF_PAIRS = 0, REF_GROUP = 1, REF_ENCODE = 2, REF_CACHED = 3 };
struct RefGroup { int mode; int G; const int32_t* ref_index; float* rows; };

// What is true of ONE call only.  The entry fills it in and forward() passes it down by const reference; nothing of it is kept on the
// handle, so no call -- refused, failed or finished -- leaves any of it behind for the next one.  (What the ABI makes sticky between
// calls -- trace, iqa_token, dbg_stop, prof_mask, the fp8 scale state -- and what is a resource stay in vtq_engine.)
struct Call {
    const char* who = nullptr;                 // the entry's name
    int nimg = 2;                              // images per item: 1 = single images, 2 = (ref, dist), 3 = (ref, dist1, dist2) triplet
    bool tokens_in = false;                    // `in` holds (B, N, H) feature rows (transformer.py:534-535), not 5-D patches
    const float *in[3] = {}, *pos[3] = {}, *scales[3] = {};      // per image (the embedding launches read slot 1 with nimg = 1 too: NULL)
    int B = 0, N = 0;                          // B items of N patches per image, or
    bool varlen = false;                       //   variable length (a NULL count array is refused by submit(), so the entry says which it is)
    const int32_t* n_img[2] = {};              //   variable length (HOST arrays): item i of image k has n_img[k][i] patches -- image 0 holds rg.G
    int64_t sumN[2] = {};                      //   items with REF_GROUP, else B; vtq_forward_varlen passes ONE array for both images.  Their sums
    int maxN = 0;                              //   per image and the maximum over all
    float* q_out = nullptr;
    // vtq_forward_vit: encoder_norm of `rows` rows per image; per-layer residual rows and attention probabilities (optional)
    float *out = nullptr, *states = nullptr, *probs = nullptr;
    int rows = 0;
    bool rollout = false;                      // the caller asked for the maps (the *_rollout* entries): rollout_out [+ last_attention_out]
    float *rollout_out = nullptr, *last_attention_out = nullptr;
    bool null_arrays = false;                  // the triplet entries: a pointer array itself was NULL
    RefGroup rg{REF_PAIRS, 0, nullptr, nullptr};
    bool calibrating = false;                  // fp8 mode: this forward chooses the activation scales (set by forward(), see kSPatch)
};

// One fp8 producer stage (a kernel that writes e4m3 activation bytes with scale `sc`).  Normal forwards: run it once, saturation
// reported into the error word.  Calibration forward: run it reporting max |value|, read that (the one place a forward
// synchronises), choose `sc`, run it again with the final scale.  launch(scale, obs) must be idempotent.
template <typename F>
int fp8_stage(vtq_engine* e, const Call& c, hipStream_t s, float& sc, F launch) {
    if (!c.calibrating) return launch(sc, Fp8Obs{nullptr, e->err_flag});
    HIP_TRY(hipMemsetAsync(e->amax_slot, 0, 4, s));
    if (launch(sc, Fp8Obs{e->amax_slot, nullptr})) return 1;
    float m = 0.f;
    HIP_TRY(hipMemcpyAsync(&m, e->amax_slot, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    sc = fp8_pick_scale(m, sc);
    return launch(sc, Fp8Obs{nullptr, e->err_flag});
}

// One call's host-built table of `ints` ints -> e->vl_tab: through the engine's pinned image, ONE copy on `s` ahead of the first launch
// that reads it, recorded in vl_uploaded, which the next call waits for before it rewrites the image.  fill(image) writes the ints.
// The workspace must be reserved first (the table lives in it).
template <typename F>
int upload_table(vtq_engine* e, const char* who, size_t ints, hipStream_t s, F fill) {
    if ((int64_t)ints > varlen_table_ints(e->capB * 2, e->capN + e->T, e->H)) return fail("%s: table of %zu ints exceeds the reserved workspace", who, ints);
    if (!e->vl_uploaded) HIP_TRY(hipEventCreateWithFlags(&e->vl_uploaded, hipEventDisableTiming));
    else HIP_TRY(hipEventSynchronize(e->vl_uploaded));      // the previous call's upload has read the image (long done, as a rule)
    if (e->vl_host_ints < ints) {
        if (e->vl_host) (void)hipHostFree(e->vl_host);
        e->vl_host = nullptr; e->vl_host_ints = 0;
        HIP_TRY(hipHostMalloc((void**)&e->vl_host, ints * sizeof(int), hipHostMallocDefault));
        e->vl_host_ints = ints;
    }
    fill(e->vl_host);
    HIP_TRY(hipMemcpyAsync(e->vl_tab, e->vl_host, ints * sizeof(int), hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(e->vl_uploaded, s));
    return 0;
}

// Where one call's device tables lie in e->vl_tab (Table): sequence j is the len[j] rows from row0[j]; `blocks`: attention_varlen.hip.  All
// NULL / 0: a uniform call, addressed by its Geometry alone.  ref_index: the group / cached forms of either kind
struct VarLen { const int* row0; const int* len; const int* blocks; int nblocks; const int* ref_index; };

// All encoder layers for the g.nseq sequences, enqueued on s.  vl.row0 != NULL: sequences of different lengths (g.S = the largest)
int run_encoder(vtq_engine* e, const Call& call, const Geometry& g, hipStream_t s, bool prune, const VarLen& vl) {
    const vtq_config& c = e->cfg;
    const int H = e->H, Md = e->Mdim, T = e->T, L = c.num_layers, f16 = e->f16, apl = e->apl, Hqp = (int)e->Hqp;
    const Num lin = e->lin;
    const int M = (int)g.M_pad;
    float* x = e->x;
    // the two activation buffers, as planes of row length ld.  QKV (ld 3H) and the MLP hidden (ld M) alias in `big`: never live together
    auto lnv = [&](int ld) { return View{e->lnbuf, e->ln_plane, ld}; };
    auto bigv = [&](int ld) { return View{e->big, e->big_plane, ld}; };
    // layer i's QKV planes: in `big`, or (vtq_forward_rollout) in a buffer of the layer's own, where Q and K survive the forward
    const bool rollout = call.rollout;
    auto qkvv = [&](int i) { return rollout ? View{e->ro_qkv[i], e->ro_plane, 3 * H} : bigv(3 * H); };
    float *xcls = e->xcls, *lncls = e->lncls, *qcls = e->qcls;
    const int64_t trace_stride = (int64_t)g.nseq * T * H;
    // LayerNorm inside the residual GEMMs (gemm_rowln.hip): the out-proj launch also writes LayerNorm 2's planes, the fc2 launch the
    // NEXT layer's LayerNorm 1 planes; only layer 0's LayerNorm 1 (behind the patch embedding) is a launch of its own.  Not while a
    // test stops the encoder between stages (vtq_debug_stop_after addresses the separate stages).
    const bool fused = e->fuse_ln && e->dbg_stop < 0;
    // fp8 mode (VTQ_PREC_FP8): LayerNorm / attention / GELU outputs are e4m3 bytes with the scales s_* (`sc`; see kSPatch), weights
    // are e4m3 rows with per-output-channel scales (de-scaled in the GEMM epilogue); the QKV output is one fp16 plane
    const bool f8m = e->fp8;
    // lnbuf = LayerNorm(x; w, b) for all M rows
    auto layernorm = [&](const float* w, const float* b, float& sc) -> int {
        Prof p(e, s, VTQ_K_LN);
        if (f8m)
            return fp8_stage(e, call, s, sc, [&](float v, Fp8Obs ob) {
                HIP_TRY(launch_layernorm(x, w, b, e->lnbuf, e->ln_plane, M, H, 2, 1, s, v, ob));
                return 0;
            });
        HIP_TRY(launch_layernorm(x, w, b, e->lnbuf, e->ln_plane, M, H, f16, apl, s));
        return 0;
    };
    // One residual branch: x += gamma * h, h = A W^T + b (A: activations scaled by 1 / ascale_inv in fp8 mode).
    //   fused: the same launch also writes lnbuf = LayerNorm(x; lnw, lnbias) (lnw NULL: none).
    //   Adapter pair 0 at `site` (transformer.py:279-283): h <- h + up(gelu(down(h))) BEFORE LayerScale and the residual add.  The
    //   residual GEMM already added gamma * h; the adapter's delta follows as two more GEMMs from h's own planes, written first into
    //   `spare` (the activation buffer A is not in): down (N = H/4 padded to the tile, GELU epilogue) into A's buffer, which is
    //   consumed by then, up (K = the padded H/4) with the same LayerScale into x.
    const bool adapters = c.num_adapters > 0;
    auto residual = [&](View a, View spare, const Lin& l, float ascale_inv, const float* gamma, const float* lnw, const float* lnbias,
                        const Layer& Ly, int site) -> int {
        const View h{spare.p, spare.plane, H}, t{a.p, a.plane, Hqp};
        if (adapters) HIP_TRY(launch_gemm(gemm_args(a, l, M, h, ascale_inv), lin, EPI_BIAS, s));
        if (fused) {
            RowLnArgs r{};
            r.A = a.p; r.a_plane = a.plane; r.lda = a.ld; r.W = l.w; r.w_plane = l.plane; r.M = M; r.N = H; r.K = l.K; r.bias = l.b;
            r.gamma = gamma; r.x = x; r.ln_w = lnw; r.ln_b = lnbias; r.out = e->lnbuf; r.o_plane = e->ln_plane;
            HIP_TRY(launch_gemm_rowln(r, lin, s));
        } else {
            GemmArgs r = gemm_args(a, l, M, View{}, ascale_inv);
            r.gamma = gamma; r.x = x;
            HIP_TRY(launch_gemm(r, lin, EPI_RESID, s));
        }
        if (adapters) {
            HIP_TRY(launch_gemm(gemm_args(h, Ly.ad_dn[site], M, t), lin, EPI_BIAS_GELU, s));
            GemmArgs u = gemm_args(t, Ly.ad_up[site], M);
            u.gamma = gamma; u.x = x;
            HIP_TRY(launch_gemm(u, lin, EPI_RESID, s));
        }
        return 0;
    };
    for (int i = 0; i < L; ++i) {
        const Layer& Ly = e->layers[i];
        const bool tail = prune && i == L - 1;
        if (!(fused && i > 0) && !tail && layernorm(Ly.ln1w, Ly.ln1b, e->s_ln1[i])) return 1;
        if (tail && rollout) {
            // vtq_forward_rollout: the rollout needs this layer's Q and K planes of every row, which the tail below never forms (see
            // rollout_workspace).  LayerNorm 1 into lnbuf (free here: the tail reads x) and the query | key rows of the QKV GEMM; x is not touched
            if (layernorm(Ly.ln1w, Ly.ln1b, e->s_ln1[i])) return 1;
            Prof p(e, s, VTQ_K_QKV);
            HIP_TRY(launch_gemm(gemm_args(lnv(H), lin_rows(Ly.qkv, 0, 2 * H), M, qkvv(i)), lin, EPI_BIAS, s));
        }
        if (tail) {
            // ---- last layer: the R consumed rows only (cls_tail.hip).  Their one query per head is folded into the key and value
            // projections, so no other row is normalised or projected: the attention streams the fp32 residual rows themselves
            const int R = g.nseq;
            {
                Prof p(e, s, VTQ_K_HEAD);
                // skinny MFMA stages on the R CLS rows (skinny.hip); activations between them as planes in the encoder's format
                const View tlv{e->tl, e->tl_plane, H}, thv{e->th, e->th_plane, Md};
                const PlaneOut tl{e->tl, e->tl_plane, H, f16, apl, nullptr};       // every row kernel of the tail writes its consumer's planes
                HIP_TRY(launch_rows_ln(x + (int64_t)e->iqa_token * H, (int64_t)g.S_pad * H, Ly.ln1w, Ly.ln1b, lncls, xcls, R, H, tl, s, vl.row0));
                {   // query projection: rows 0 .. H-1 of the packed QKV weight
                    SkinnyArgs a = skinny_args(tlv, lin_rows(Ly.qkv, 0, H), R, apl);
                    a.epi = SK_PLAIN; a.y = qcls; a.ldy = H; a.ycols = H;
                    HIP_TRY(launch_skinny(a, lin, s));
                }
                {   // u = W_k^T q (rows H .. 2H-1 of the packed QKV weight; q . b_k is constant per head); zbar = softmax-weighted LayerNorm rows
                    const Lin wk = lin_rows(Ly.qkv, H, H);
                    const PlaneOut zo{e->fold_z, e->fold_z_plane, (H / 64) * H, f16, apl, nullptr};
                    HIP_TRY(launch_cls_fold(qcls, wk.w, wk.plane, wk.K, f16, e->wpl, x, (int64_t)g.S_pad * H, Ly.ln1w, Ly.ln1b, e->fold_u, e->fold_part,
                                            R, g.S, H, zo, s, e->att.terms == 3, VarSeq{vl.row0, vl.len}));
                }
                {   // value projection: ctx[64h ..] = W_v,h zbar_h + b_v (rows 2H .. 3H-1), head h reading columns h H .. of its row
                    SkinnyArgs a = skinny_args(View{e->fold_z, e->fold_z_plane, (H / 64) * H}, lin_rows(Ly.qkv, 2 * H, H), R, apl);
                    a.xcol64 = H; a.epi = SK_PLAIN; a.ya = e->tl; a.ya_plane = e->tl_plane; a.ldya = H;
                    HIP_TRY(launch_skinny(a, lin, s));
                }
                {   // out-proj + LayerScale + residual, in place on the CLS rows
                    SkinnyArgs a = skinny_args(tlv, Ly.out, R, apl);
                    a.epi = SK_RESID; a.gamma = Ly.g1; a.res = xcls; a.ldr = H; a.y = xcls; a.ldy = H; a.ycols = H;
                    HIP_TRY(launch_skinny(a, lin, s));
                }
                HIP_TRY(launch_rows_ln(xcls, H, Ly.ln2w, Ly.ln2b, lncls, nullptr, R, H, tl, s));
                {   // fc1 + GELU -> planes
                    SkinnyArgs a = skinny_args(tlv, Ly.fc1, R, apl);
                    a.epi = SK_GELU; a.ya = e->th; a.ya_plane = e->th_plane; a.ldya = Md;
                    HIP_TRY(launch_skinny(a, lin, s));
                }
                {   // fc2 + LayerScale + residual
                    SkinnyArgs a = skinny_args(thv, Ly.fc2, R, apl);
                    a.epi = SK_RESID; a.gamma = Ly.g2; a.res = xcls; a.ldr = H; a.y = xcls; a.ldy = H; a.ycols = H;
                    HIP_TRY(launch_skinny(a, lin, s));
                }
            }
            break;
        }
        if (e->dbg_stop == i * 7 + 0) return 0;
        {
            Prof p(e, s, VTQ_K_QKV);
            HIP_TRY(launch_gemm(gemm_args(lnv(H), Ly.qkv, M, qkvv(i), 1.0f / e->s_ln1[i]), lin, EPI_BIAS, s));
        }
        if (e->dbg_stop == i * 7 + 1) return 0;
        {
            Prof p(e, s, VTQ_K_ATTN);
            const View qv = qkvv(i);
            if (f8m) {
                if (fp8_stage(e, call, s, e->s_att[i], [&](float sc, Fp8Obs ob) { HIP_TRY(launch_attention(e->big, e->big_plane, e->lnbuf, e->ln_plane, g.nseq, g.S, g.S_pad, H, e->att, s, sc, ob, e->att.terms == 3)); return 0; })) return 1;
            } else if (vl.blocks) HIP_TRY(launch_attention_varlen(qv.p, qv.plane, e->lnbuf, e->ln_plane, vl.blocks, vl.nblocks, H, e->att, s, e->att.terms == 3));
            else HIP_TRY(launch_attention(qv.p, qv.plane, e->lnbuf, e->ln_plane, g.nseq, g.S, g.S_pad, H, e->att, s, 0.0f, Fp8Obs{nullptr, nullptr}, e->att.terms == 3));
            // forward_vit's attention maps: from the same QKV planes, before the out-proj (with adapters it reuses `big`)
            if (call.probs)
                HIP_TRY(launch_attention_probs(qv.p, qv.plane, call.probs + (int64_t)i * g.nseq * (H / 64) * g.S * g.S, g.nseq, g.S, g.S_pad, H,
                                               e->att, s, e->att.terms == 3));
        }
        if (e->dbg_stop == i * 7 + 2) return 0;
        {   // x += ls1 * out-proj(attention); fused: lnbuf = LayerNorm 2 (x).  QKV is consumed: `big` is the spare buffer
            Prof p(e, s, VTQ_K_OUTPROJ);
            if (residual(lnv(H), bigv(H), Ly.out, 1.0f / e->s_att[i], Ly.g1, Ly.ln2w, Ly.ln2b, Ly, 0)) return 1;
        }
        if (e->dbg_stop == i * 7 + 3) return 0;
        if (!fused && layernorm(Ly.ln2w, Ly.ln2b, e->s_ln2[i])) return 1;
        if (e->dbg_stop == i * 7 + 4) return 0;
        {
            Prof p(e, s, VTQ_K_FC1);
            const GemmArgs a = gemm_args(lnv(H), Ly.fc1, M, bigv(Md), 1.0f / e->s_ln2[i]);
            if (f8m) {
                if (fp8_stage(e, call, s, e->s_gelu[i], [&](float sc, Fp8Obs ob) { GemmArgs b = a; b.out_scale = sc; b.obs = ob; HIP_TRY(launch_gemm(b, lin, EPI_BIAS_GELU, s)); return 0; })) return 1;
            } else HIP_TRY(launch_gemm(a, lin, EPI_BIAS_GELU, s));
        }
        if (e->dbg_stop == i * 7 + 5) return 0;
        {   // x += ls2 * fc2(hidden); fused: lnbuf = the next layer's LayerNorm 1 (x) (none behind the last layer: final_diff normalises
            // the CLS rows).  LayerNorm 2's planes are consumed: `lnbuf` is the spare buffer
            Prof p(e, s, VTQ_K_FC2);
            const Layer* nx = (i + 1 < L) ? &e->layers[i + 1] : nullptr;
            if (prune && i + 1 == L - 1) nx = nullptr;              // the CLS-only last layer normalises the rows it reads itself
            if (residual(bigv(Md), lnv(H), Ly.fc2, 1.0f / e->s_gelu[i], Ly.g2, nx ? nx->ln1w : nullptr, nx ? nx->ln1b : nullptr, Ly, 1)) return 1;
        }
        if (e->dbg_stop == i * 7 + 6) return 0;
        if (e->trace) HIP_TRY(launch_copy_tokens(x, e->trace + (i + 1) * trace_stride, g.nseq, g.sm, T, H, s));
        if (call.states) HIP_TRY(launch_copy_tokens(x, call.states + (int64_t)i * g.nseq * call.rows * H, g.nseq, g.sm, call.rows, H, s));
    }
    return 0;
}

// PReLU slope of the head's first consumer (the first RCAB), or NULL when there is no decoder
const float* head_first_slope(const vtq_engine* e) { return (e->cfg.calibrate && !e->rgs.empty()) ? e->rgs[0].rcabs[0].slope : nullptr; }

// DiffNet head + quality predictor on d[HB][H] (the CLS difference after diff_scale; vtamiq.py:111-117,
// channel_attention.py:13-86) as a chain of skinny MFMA stages (skinny.hip), fp16 hi/lo operands, fp32 everywhere else.
//   RCAB (channel_attention.py:41-50, 77-86) = two stages with the CA squeeze folded into the conv (launch_fold_ca):
//     [c | t] = [Wc ; Wd Wc] prelu(r) + bcat, t = relu(.)        y = r + c * sigmoid(Wu t + bu)
//   Every stage writes the planes its consumer reads, already passed through the consumer's PReLU.
int run_head(vtq_engine* e, const float* d, int HB, float* q_out, hipStream_t s, bool planes_ready = false) {
    const vtq_config& c = e->cfg;
    const int H = e->H;
    const Num h3{1, 3};
    if (HB > e->r_alloc) return fail("run_head: %d rows exceed the reserved %d", HB, e->r_alloc);
    auto stage = [&](void* xa, int64_t xpl, int ldx, const Lin& L) { return skinny_args(View{xa, xpl, ldx}, L, HB, 2); };
    void *pin = e->hp[0], *pout = e->hp[1];
    if (!planes_ready) HIP_TRY(launch_rows_to_planes(d, H, head_first_slope(e), pin, e->hp_plane, H, HB, H, 1, 2, s));
    if (c.calibrate) {
        const float* xr = d;                 // residual-group input (fp32)
        float* xr_buf[2] = {e->hb[1], e->hb[0]};      // d lives in hb[0]: the first RG writes hb[1]
        float *y0 = e->hb[2], *y1 = e->hb[3], *cb = e->hb[4];
        const size_t ng = e->rgs.size();
        for (size_t gi = 0; gi < ng; ++gi) {
            Rg& R = e->rgs[gi];
            const float* y = xr;
            float* yo = y0;
            const size_t nr = R.rcabs.size();
            for (size_t k = 0; k < nr; ++k) {
                Rcab& r = R.rcabs[k];
                {
                    SkinnyArgs a = stage(pin, e->hp_plane, H, r.cat);
                    a.epi = SK_CONVCAT; a.nsplit = H; a.y = cb; a.ldy = H; a.ycols = H;
                    a.ya = e->ht; a.ya_plane = e->ht_plane; a.ldya = e->hidp; a.pcol0 = H;
                    HIP_TRY(launch_skinny(a, h3, s));
                }
                {
                    SkinnyArgs a = stage(e->ht, e->ht_plane, e->hidp, r.up);
                    a.epi = SK_GATE; a.res = y; a.aux = cb; a.ldr = H; a.y = yo; a.ldy = H; a.ycols = H;
                    a.ya = pout; a.ya_plane = e->hp_plane; a.ldya = H;
                    a.next_slope = (k + 1 < nr) ? R.rcabs[k + 1].slope : nullptr;      // the RG tail conv takes y itself
                    HIP_TRY(launch_skinny(a, h3, s));
                }
                y = yo;
                yo = (yo == y0) ? y1 : y0;
                std::swap(pin, pout);
            }
            {   // x + Conv1d(body(x))   (channel_attention.py:28-29; DropPath is identity in eval)
                float* xn = xr_buf[gi & 1];
                SkinnyArgs a = stage(pin, e->hp_plane, H, R.tail);
                a.epi = SK_RESID; a.res = xr; a.ldr = H; a.y = xn; a.ldy = H; a.ycols = H;
                a.ya = pout; a.ya_plane = e->hp_plane; a.ldya = H;
                a.next_slope = (gi + 1 < ng) ? e->rgs[gi + 1].rcabs[0].slope : nullptr;
                HIP_TRY(launch_skinny(a, h3, s));
                xr = xn;
                std::swap(pin, pout);
            }
        }
        {   // final Conv1d of the decoder (vtamiq.py:22): only the planes for the predictor are needed
            SkinnyArgs a = stage(pin, e->hp_plane, H, e->qd);
            a.epi = SK_PLAIN; a.ya = pout; a.ya_plane = e->hp_plane; a.ldya = H;
            HIP_TRY(launch_skinny(a, h3, s));
            std::swap(pin, pout);
        }
    }
    {   // q_predictor (vtamiq.py:71-77): Linear(H, H/4) -> PReLU -> Linear(H/4, 1)
        SkinnyArgs a = stage(pin, e->hp_plane, H, e->p1);
        a.epi = SK_PRELU; a.post_slope = e->p2a; a.ya = e->hq; a.ya_plane = e->hq_plane; a.ldya = H / 4;
        HIP_TRY(launch_skinny(a, h3, s));
        SkinnyArgs b = stage(e->hq, e->hq_plane, H / 4, e->p4);
        b.epi = SK_PLAIN; b.y = q_out; b.ldy = 1; b.ycols = 1;
        HIP_TRY(launch_skinny(b, h3, s));
    }
    return 0;
}

int all_loaded(const vtq_engine* e, const char* who) {
    for (auto& kv : e->slots)
        if (!kv.second.loaded) return fail("%s: weight '%s' was never loaded", who, kv.first.c_str());
    return 0;
}

int null_handle(const char* who) { return fail("%s: null handle", who); }

}  // namespace

extern "C" {

int vtq_abi_version(void) { return VTQ_ABI_VERSION; }
const char* vtq_last_error(void) { return g_err.c_str(); }

int vtq_create(const vtq_config* cfg, vtq_handle* out) {
    if (!cfg || !out) return fail("vtq_create: null argument");
    const vtq_config& c = *cfg;
    if (c.hidden_size != 768 && c.hidden_size != 1024) return fail("hidden_size %d unsupported (768 | 1024)", c.hidden_size);
    if (c.num_heads <= 0 || c.hidden_size / c.num_heads != 64 || c.hidden_size % c.num_heads)
        return fail("head_dim must be 64 (hidden %d, heads %d)", c.hidden_size, c.num_heads);
    if (c.mlp_dim % 256 || c.mlp_dim <= 0) return fail("mlp_dim %d must be a positive multiple of 256", c.mlp_dim);
    if (c.num_adapters < 0 || c.num_adapters > 64) return fail("num_adapters %d", c.num_adapters);
    if (c.num_adapters > 0 && c.precision == VTQ_PREC_FP8) return fail("adapters are not available in the fp8 mode (the adapter input would need an e4m3 copy)");
    if (c.patch_dim != 768 && c.patch_dim != 192) return fail("patch_dim %d unsupported (3*16*16 or 3*8*8)", c.patch_dim);
    if (c.num_layers < 1 || c.pos_grid < 1 || c.num_extra_tokens < 0) return fail("bad topology");
    if (c.options & ~(VTQ_OPT_FULL_LAST_LAYER | VTQ_OPT_FP8_STATIC_SCALES | VTQ_OPT_FUSED_LAYERNORM)) return fail("unknown vtq_config.options bits 0x%x", c.options);
    if ((c.options & VTQ_OPT_FUSED_LAYERNORM) && (c.mlp_dim % 32 || c.mlp_dim < 128)) return fail("VTQ_OPT_FUSED_LAYERNORM needs mlp_dim %% 32 == 0 and >= 128");
    if (c.calibrate && (c.num_rgs < 1 || c.num_rcabs < 1 || c.ca_hidden < 4 || c.ca_hidden % 4 || c.ca_hidden > 256))
        return fail("bad DiffNet topology (rgs %d, rcabs %d, ca_hidden %d)", c.num_rgs, c.num_rcabs, c.ca_hidden);
    vtq_engine* e = new vtq_engine();
    e->cfg = c;
    switch (c.precision) {
        case VTQ_PREC_BF16:   e->lin = Num{0, 1}; e->att = Num{0, 1}; break;
        case VTQ_PREC_BF16X3: e->lin = Num{0, 3}; e->att = Num{0, 3}; break;
        case VTQ_PREC_FP16:   e->lin = Num{1, 1}; e->att = Num{1, 1}; break;
        case VTQ_PREC_FP16X3: e->lin = Num{1, 3}; e->att = Num{1, 3}; break;
        case VTQ_PREC_FP16X2: e->lin = Num{1, 2}; e->att = Num{1, 3}; break;     // attention keeps the 3-term form
#ifdef VTQ_WITH_FP8
        case VTQ_PREC_FP8:    e->lin = Num{2, 1}; e->att = Num{1, 1}; e->fp8 = true; break;   // e4m3 linears, single-fp16 attention (2e-4 << the e4m3 step)
#else
        case VTQ_PREC_FP8:    delete e; return fail("precision 5 (fp8) is an experiment that this library was built without: build it with python -m vtamiq_amd.build --fp8 "
                                                    "(include/vtamiq_hip_fp8.h, vtamiq_amd/experimental_fp8.py)");
#endif
        default: delete e; return fail("unknown precision %d", c.precision);
    }
    e->f16 = e->fp8 ? 1 : e->lin.f16;          // fp8 mode: the QKV output is one fp16 plane (buffers are sized for it);
    e->apl = e->fp8 ? 1 : e->lin.apl();        //   LayerNorm / GELU / attention outputs are e4m3 bytes
    e->wpl = e->lin.wpl();
    e->H = c.hidden_size;
    e->Mdim = c.mlp_dim;
    e->T = 1 + c.num_extra_tokens;
    e->cls_prune = !(c.options & VTQ_OPT_FULL_LAST_LAYER);
    e->fuse_ln = (c.options & VTQ_OPT_FUSED_LAYERNORM) != 0;
    if (e->fuse_ln && !(c.hidden_size == 768 && !e->fp8 && e->lin.terms == 3 && c.num_adapters == 0)) {
        delete e;
        return fail("VTQ_OPT_FUSED_LAYERNORM needs hidden_size 768, a 3-term precision (fp16x3 / bf16x3) and no adapters");
    }
    e->s_ln1.assign(c.num_layers, kSLn); e->s_att.assign(c.num_layers, kSAtt); e->s_ln2.assign(c.num_layers, kSLn); e->s_gelu.assign(c.num_layers, kSGelu);
    e->fp8_static = (c.options & VTQ_OPT_FP8_STATIC_SCALES) != 0;
    e->ro_qkv.assign(c.num_layers, nullptr);
    if (hipMalloc((void**)&e->err_flag, 16) != hipSuccess || hipMemset(e->err_flag, 0, 16) != hipSuccess) {
        vtq_destroy(e);
        return fail("vtq_create: device allocation failed");
    }
    e->allocs.push_back(e->err_flag);
    e->amax_slot = (float*)(e->err_flag + 2);           // same 16-byte allocation
    if (hipHostMalloc((void**)&e->err_host, 64, hipHostMallocDefault) != hipSuccess) {
        e->err_host = nullptr;
        vtq_destroy(e);
        return fail("vtq_create: pinned host allocation failed");
    }
    if (build(e)) { vtq_destroy(e); return 1; }
    *out = e;
    return 0;
}

void vtq_destroy(vtq_handle e) {
    if (!e) return;
    (void)hipDeviceSynchronize();
    for (void* p : e->allocs) (void)hipFree(p);
    if (e->err_host) (void)hipHostFree(e->err_host);
    if (e->vl_host) (void)hipHostFree(e->vl_host);
    if (e->vl_uploaded) (void)hipEventDestroy(e->vl_uploaded);
    for (void* p : e->ws_allocs) (void)hipFree(p);
    for (void* p : e->ro_allocs) (void)hipFree(p);
    for (auto& ev : e->ev_used) { (void)hipEventDestroy(ev.a); (void)hipEventDestroy(ev.b); }
    for (auto& ev : e->ev_free) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    delete e;
}

int vtq_load_weights(vtq_handle e, const vtq_tensor_desc* descs, int32_t n, void* stream) {
    if (!e || !descs) return fail("vtq_load_weights: null argument");
    hipStream_t s = (hipStream_t)stream;
    float* scratch = nullptr;                                  // one buffer for the scaled copies, reused in stream order
    int64_t scratch_n = 0;
    struct Free { float*& p; ~Free() { if (p) { (void)hipDeviceSynchronize(); (void)hipFree(p); } } } free_scratch{scratch};
    for (int i = 0; i < n; ++i) {
        const vtq_tensor_desc& d = descs[i];
        if (!d.name || !d.data) return fail("vtq_load_weights: descriptor %d has a null field", i);
        auto it = e->slots.find(d.name);
        if (it == e->slots.end()) return fail("vtq_load_weights: unexpected tensor '%s'", d.name);
        Slot& sl = it->second;
        if (sl.numel != d.numel) return fail("vtq_load_weights: '%s' has %lld elements, expected %lld", d.name, (long long)d.numel, (long long)sl.numel);
        if (sl.ignore) { sl.loaded = true; continue; }
        const float* src = (const float*)d.data;
        if (sl.mul != 1.0f) {                                   // scaled copy first (query projection, 3-term attention)
            if (scratch_n < sl.numel) {
                if (scratch) (void)hipFree(scratch);
                scratch = nullptr;
                HIP_TRY(hipMalloc((void**)&scratch, (size_t)sl.numel * 4));
                scratch_n = sl.numel;
            }
            HIP_TRY(launch_scale_copy(src, scratch, sl.numel, sl.mul, s));
            src = scratch;
        }
        if (sl.split && e->fp8) HIP_TRY(launch_quant_rows_fp8(src, sl.dst, sl.scale, (int)(sl.numel / sl.K), (int)sl.K, s, (int)sl.Kp));
        else if (sl.split && sl.Kp != sl.K)
            HIP_TRY(launch_split_rows_pad(src, sl.dst, sl.plane, (int)(sl.numel / sl.K), (int)sl.K, (int)sl.Kp, e->f16, e->wpl, s));
        else if (sl.split) HIP_TRY(launch_split(src, sl.dst, sl.plane, sl.numel, e->f16, e->wpl, s));
        else HIP_TRY(hipMemcpyAsync(sl.dst, src, (size_t)sl.numel * 4, hipMemcpyDeviceToDevice, s));
        sl.loaded = true;
    }
    if (pack_head(e, s)) return 1;
    HIP_TRY(hipStreamSynchronize(s));
    // fp8 mode: scales calibrated on the previous weights do not fit these (activations would clamp at +-448): the next forward
    // calibrates again -- unless the caller installed the scales itself (a checkpoint that carries them; vtq_fp8_set_scales)
    if (e->fp8 && !e->fp8_installed) e->fp8_calibrated = false;
    return 0;
}

size_t vtq_workspace_bytes(vtq_handle e, int32_t B, int32_t N) { return e ? ws_bytes(workspace(e, B, N)) : 0; }

int vtq_reserve(vtq_handle e, int32_t B, int32_t N) {
    if (!e || B < 1 || N < 1) return fail("vtq_reserve: bad argument");
    return reserve(e, B, N);
}

int vtq_set_token_trace(vtq_handle e, float* buf) {
    if (!e) return null_handle("vtq_set_token_trace");
    e->trace = buf;
    return 0;
}

int vtq_set_iqa_token(vtq_handle e, int32_t token) {
    if (!e) return null_handle("vtq_set_iqa_token");
    if (token < 0 || token > e->cfg.num_extra_tokens)
        return fail("vtq_set_iqa_token: token %d outside [0, %d] (CLS + num_extra_tokens register tokens)", (int)token, (int)e->cfg.num_extra_tokens);
    e->iqa_token = token;
    return 0;
}

int vtq_debug_stop_after(vtq_handle e, int32_t stage) {
    if (!e) return null_handle("vtq_debug_stop_after");
    e->dbg_stop = stage;
    return 0;
}

int vtq_debug_buffers(vtq_handle e, void** x, void** lnbuf, void** big, int64_t* rows) {
    if (!e || !e->x) return fail("vtq_debug_buffers: no workspace yet (run a forward first)");
    if (x) *x = e->x;
    if (lnbuf) *lnbuf = e->lnbuf;
    if (big) *big = e->big;
    if (rows) *rows = e->ln_plane / e->H;
    return 0;
}

int vtq_debug_attention_variant(int32_t v) {
    attention_set_variant(v);
    return 0;
}

int vtq_debug_gemm_variant(int32_t v) {
    if (v < GEMM_TILE_AUTO || v > 31) return fail("vtq_debug_gemm_variant: %d", v);
    gemm_set_variant(v);
    return 0;
}

int vtq_debug_cu_partition(int32_t gemm_cus_per_xcd, int32_t attention_cus) {
    if (gemm_cus_per_xcd < 0 || gemm_cus_per_xcd > 32 || attention_cus < 0 || attention_cus > 4096) return fail("vtq_debug_cu_partition: %d, %d", (int)gemm_cus_per_xcd, (int)attention_cus);
    gemm_set_cus_per_xcd(gemm_cus_per_xcd);
    attention_set_cus(attention_cus);
    return 0;
}

int vtq_debug_attention_map(int32_t m) {
    if (m < 0 || m > 1) return fail("vtq_debug_attention_map: %d", (int)m);
    attention_set_map(m);
    return 0;
}

int vtq_debug_cu_map(uint32_t* out, int32_t nblocks, int32_t spin_us, void* stream) {
    if (!out || nblocks < 1 || nblocks > 4096 || spin_us < 0 || spin_us > 100000) return fail("vtq_debug_cu_map: bad argument");
    HIP_TRY(launch_cu_map(out, nblocks, spin_us, (hipStream_t)stream));
    return 0;
}

int vtq_k_gemm_tile_rule(int32_t M, int32_t N, int32_t K, int32_t num) {
    const Num nm = num_from_code(num);
    if (!num_valid(nm)) return -1;
    return gemm_tile_rule(M, N, K, nm);
}

int vtq_k_attention_rule(int32_t nseq, int32_t S_pad, int32_t H, int32_t num, int32_t cus) {
    const Num nm = num_from_code(num);
    if (!num_valid(nm)) return -1;
    return attention_rule(nseq, S_pad, H, nm.terms, cus);
}

int vtq_debug_gemm_diag(void*, int32_t) {
    return 0;
}

int vtq_debug_mfma_stream(int32_t f16, int32_t data, double warm_s, double timed_s, double* tflops, double* ghz, void* stream) {
    if (f16 < 0 || f16 > 1 || data < 0 || data > 2 || !(warm_s >= 0.0) || !(timed_s > 0.0) || warm_s > 30.0 || timed_s > 30.0 || !tflops)
        return fail("vtq_debug_mfma_stream: bad argument");
    HIP_TRY(mfma_stream_measure(f16, data, warm_s, timed_s, tflops, ghz, (hipStream_t)stream));
    return 0;
}

int vtq_profile_enable(vtq_handle e, uint32_t mask) {
    if (!e) return null_handle("vtq_profile_enable");
    e->prof_mask = mask;
    return 0;
}

int vtq_profile_collect(vtq_handle e, double* ms_sum, int64_t* launches) {
    if (!e || !ms_sum || !launches) return fail("vtq_profile_collect: null argument");
    for (int k = 0; k < VTQ_K_COUNT; ++k) { ms_sum[k] = 0; launches[k] = 0; }
    for (auto& ev : e->ev_used) {
        HIP_TRY(hipEventSynchronize(ev.b));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
        ms_sum[ev.cls] += ms;
        launches[ev.cls] += 1;
        e->ev_free.push_back({ev.a, ev.b});
    }
    e->ev_used.clear();
    return 0;
}

// Attention rollout of the consumed token behind a forward that kept every layer's Q / K planes (e->ro_qkv): one step per layer, last to
// first, every launch on s.  The walk starts at r = e_token, so the first step's per-head sums are the last layer's attention row of the
// token: last_attention.  The row vector ping-pongs between the two workspace vectors; the LAST step writes the caller's rollout_out itself
// ([nseq][S] is its layout), so there is no copy.  A variable-length call (vl.blocks) takes the table-driven step on the call's own tables: the
// vectors, the partials and both outputs are then packed like the rows (launch_rollout_step_varlen) -- g.sm.pitch is the call's row count --
// and fit what reserve_rollout(ceil(nseq / 2), maxN) holds: ro_r >= nseq * S_max >= rows, ro_part = that * heads * ceil(S_max / 128).
static int run_rollout(vtq_engine* e, const Call& c, const Geometry& g, hipStream_t s, const VarLen& vl) {
    const int H = e->H, L = e->cfg.num_layers, t = e->iqa_token;
    const bool ql = e->att.terms == 3;
    auto dst = [&](int op) { return op == L - 1 ? c.rollout_out : e->ro_r[op & 1]; };      // op 0 = the last layer ... op L - 1 = layer 0
    for (int op = 0; op < L; ++op) {
        const float* r = op ? dst(op - 1) : nullptr;
        float* last = op ? nullptr : c.last_attention_out;
        if (vl.blocks)
            HIP_TRY(launch_rollout_step_varlen(e->ro_qkv[L - 1 - op], e->ro_plane, r, t, e->ro_part, dst(op), last, vl.blocks, vl.nblocks, vl.row0,
                                               vl.len, g.nseq, g.S, g.sm.pitch, H, e->att, s, ql));
        else
            HIP_TRY(launch_rollout_step(e->ro_qkv[L - 1 - op], e->ro_plane, r, t, e->ro_part, dst(op), last, g.nseq, g.S, g.S_pad, H, e->att, s, ql));
    }
    return 0;
}

// The last step of a call: the consumed token's rows of the encoded sequences -> what the entry returns.
//   nimg = 1, REF_PAIRS (vtq_forward_vit): no head -- c.out receives encoder_norm of c.rows rows per image
//   REF_ENCODE: the rows go to the caller's cache, no head (and the rollout of its G sequences where asked for)
//   otherwise: the difference of each pair (nimg = 2: q_out[B]; nimg = 3: q_out[2B] = (ref, dist1) then (ref, dist2) with ref encoded once;
//   REF_GROUP / REF_CACHED: q_out[B], distorted image m against reference ref_index[m]), the head, and the rollout where asked for
static int finish(vtq_engine* e, const Call& c, const Geometry& g, hipStream_t s, bool prune, const VarLen& vl) {
    const int H = e->H, B = c.B, mode = c.rg.mode, ndist = c.nimg - 1;
    const int B0 = mode == REF_GROUP ? c.rg.G : B, HB = mode == REF_PAIRS ? ndist * B : B;      // sequences of image 0; head batch
    if (c.nimg == 1 && mode == REF_PAIRS) {               // encoder_norm (transformer.py:376) of the requested rows
        Prof p(e, s, VTQ_K_LN);
        HIP_TRY(launch_seq_rows_ln(e->x, e->encw, e->encb, c.out, g.nseq, g.sm, c.rows, H, s, e->err_flag));
        return 0;
    }
    {   // ---- head (vtamiq.py:104-117)
        Prof p(e, s, VTQ_K_HEAD);
        float* d = e->hb[0];
        const PlaneOut hp{e->hp[0], e->hp_plane, H, 1, 2, head_first_slope(e)};      // the first head stage's input planes
        const float* gamma = e->cfg.diff_scale ? e->diff_gamma : nullptr;
        // the consumed token's residual row of sequence j: row j of the tail's output, or token row iqa_token of sequence j in x
        const float* rows = prune ? e->xcls : e->x + (int64_t)e->iqa_token * H;
        const int64_t stride = prune ? H : (int64_t)g.S_pad * H;
        // sequences of different lengths in x (the unpruned path of a variable-length call): sequence j's row comes from the row offsets
        const int* row0 = prune ? nullptr : vl.row0;
        if (mode == REF_ENCODE) {
            HIP_TRY(launch_export_rows(rows, stride, c.rg.rows, B, H, s, e->err_flag, row0));
            return c.rollout ? run_rollout(e, c, g, s, vl) : 0;
        }
        if (mode == REF_GROUP)
            HIP_TRY(launch_group_diff(rows, stride, rows + (row0 ? 0 : B0 * stride), stride, vl.ref_index, B, e->encw, e->encb, gamma, d, H, hp, s, e->err_flag,
                                      row0, row0 ? row0 + B0 : nullptr));
        else if (mode == REF_CACHED)
            HIP_TRY(launch_group_diff(c.rg.rows, H, rows, stride, vl.ref_index, B, e->encw, e->encb, gamma, d, H, hp, s, e->err_flag, nullptr, row0));
        else if (prune) HIP_TRY(launch_final_diff(e->xcls, e->encw, e->encb, gamma, d, B, ndist, SeqMap{1, g.nseq, 0}, H, hp, s, e->err_flag));
        else HIP_TRY(launch_final_diff(e->x + (int64_t)e->iqa_token * H, e->encw, e->encb, gamma, d, B, ndist, g.sm, H, hp, s, e->err_flag, vl.row0));
        if (run_head(e, d, HB, c.q_out, s, true)) return 1;
    }
    if (c.rollout && run_rollout(e, c, g, s, vl)) return 1;
    if (c.calibrating) e->fp8_calibrated = true;
    return 0;
}

// THE forward path: every entry describes its batch as a Call, submit() refuses what has to be refused, and the call ends here.  Each step is stated once; what
// differs between the entries is read off the Call where it differs.
//   REF_GROUP: image 0 holds rg.G sequences instead of B;  the variable-length entries (n_img[0] != NULL): every sequence at its own length
static int forward(vtq_engine* e, Call c, void* stream) {
    const vtq_config& cfg = e->cfg;
    const bool varlen = c.n_img[0] != nullptr, rollout = c.rollout, tokens_in = c.tokens_in, use_scales = cfg.num_scales > 1;
    const int nimg = c.nimg, B = c.B, mode = c.rg.mode, H = e->H, T = e->T;
    const int B0 = mode == REF_GROUP ? c.rg.G : B;           // sequences of image 0
    const int nseq = B0 + (nimg - 1) * B;
    hipStream_t s = (hipStream_t)stream;
    // ---- workspace: capacity is kept in units of sequence pairs; varlen reserves an upper bound, the batch is no larger than B pairs of maxN
    if (reserve(e, (nseq + 1) / 2, varlen ? c.maxN : c.N)) return 1;
    if (rollout && reserve_rollout(e, (nseq + 1) / 2, varlen ? c.maxN : c.N)) return 1;
    // fp8 mode: the first forward of an engine calibrates the activation scales on its own batch (see kSPatch); it synchronises
    // the stream once per quantisation point and returns this batch's scores computed with the final scales
    c.calibrating = e->fp8 && !e->fp8_static && !e->fp8_calibrated && e->dbg_stop < 0;
    const Geometry g = varlen ? geometry_varlen(e, nseq, c.sumN[0] + c.sumN[1], c.maxN) : geometry_seq(e, nseq, c.N);

    // ---- the call's device table: host image, then ONE upload on `s` ahead of every launch --------------------------------------
    VarLen vl{};
    const bool indexed = mode == REF_GROUP || mode == REF_CACHED;
    if (varlen) {
        const Table tb(nseq);
        const int nref = indexed ? B : 0;
        std::vector<int> len(nseq);
        for (int j = 0; j < nseq; ++j) len[j] = (j < B0 ? c.n_img[0][j] : c.n_img[1][j - B0]) + T;
        const std::vector<int> blocks = attention_varlen_blocks(len.data(), nseq, H);
        const auto fill = [&](int* t) {
            int64_t r = 0;
            for (int j = 0; j < nseq; ++j) { t[j] = (int)r; t[tb.len + j] = len[j]; r += len[j]; }
            t[nseq] = (int)r;
            for (int m = 0; m < nref; ++m) t[tb.ref + m] = c.rg.ref_index[m];
            for (int k = tb.ref + nref; k < tb.blk; ++k) t[k] = 0;
            memcpy(t + tb.blk, blocks.data(), blocks.size() * sizeof(int));
        };
        if (upload_table(e, c.who, (size_t)tb.blk + blocks.size(), s, fill)) return 1;
        vl = VarLen{e->vl_tab, e->vl_tab + tb.len, e->vl_tab + tb.blk, (int)(blocks.size() / 4), indexed ? e->vl_tab + tb.ref : nullptr};
    } else if (indexed) {
        if (upload_table(e, c.who, (size_t)B, s, [&](int* t) { for (int m = 0; m < B; ++m) t[m] = c.rg.ref_index[m]; })) return 1;
        vl.ref_index = e->vl_tab;
    }
    {   // tile schedules of this geometry's GEMM shapes: built and uploaded here (first forward of a tile grid only; DESIGN.md section 4
        // has what bounds the cache), not inside a launch.  (M, 2H, H) is the rollout's query | key projection of the last layer; the
        // uniform entries prepare it on every call, a variable-length call exactly when it asks for a rollout
        const int wpl = e->wpl, M = (int)g.M_pad;
        HIP_TRY(gemm_prepare((int)g.P_pad, H, (int)e->PDp, wpl, s));
        HIP_TRY(gemm_prepare(M, 3 * H, H, wpl, s));
        if (!varlen || rollout) HIP_TRY(gemm_prepare(M, 2 * H, H, wpl, s));
        HIP_TRY(gemm_prepare(M, H, H, wpl, s));
        HIP_TRY(gemm_prepare(M, e->Mdim, H, wpl, s));
        HIP_TRY(gemm_prepare(M, H, e->Mdim, wpl, s));
        if (cfg.num_adapters > 0) { HIP_TRY(gemm_prepare(M, (int)e->Hqp, H, wpl, s)); HIP_TRY(gemm_prepare(M, H, (int)e->Hqp, wpl, s)); }
    }

    // ---- embeddings (transformer.py:526-562) -------------------------------------------------------------------
    // 5-D patches: packed to planes here, then one GEMM whose epilogue adds the table rows and scatters into x.  Pre-embedded input
    // (transformer.py:534-535): `in` are (B, N, H) feature rows; no patch convolution, a row kernel adds the table rows.
    // Patch rows lie (image, item, patch): N1 per image after image 0's R0 -- uniform B * N after B0 * N, varlen the sums of each image's
    // counts, the sequence map replaced by the tables, the pad rows cleared as the one run of g.sm
    {
        const int N1 = varlen ? (int)c.sumN[nimg > 1] : B * c.N, R0 = varlen ? (int)c.sumN[0] : B0 * c.N;
        Prof p(e, s, VTQ_K_CONVERT);
        if (!tokens_in && e->fp8) {
            if (fp8_stage(e, c, s, e->s_patch, [&](float sc, Fp8Obs ob) { HIP_TRY(launch_pack_patches(c.in, nimg, e->big, e->big_plane, N1, cfg.patch_dim, (int)g.P_pad, 2, 1, s, sc, (int)e->PDp, ob)); return 0; })) return 1;
        } else if (!tokens_in) HIP_TRY(launch_pack_patches(c.in, nimg, e->big, e->big_plane, N1, cfg.patch_dim, (int)g.P_pad, e->f16, e->apl, s, 1.0f, (int)e->PDp, Fp8Obs{nullptr, nullptr}, R0));
        HIP_TRY(launch_embed_index(c.pos, use_scales ? c.scales : nullptr, nimg, e->pidx, e->sidx, e->row_map, B, varlen ? N1 : c.N, (int)g.P_pad, g.sm, T,
                                   cfg.pos_grid, cfg.num_scales, e->err_flag, s, vl.row0, B0, varlen ? R0 : 0));
        HIP_TRY(launch_zero_pad_rows(e->x, g.sm.per, g.sm.pitch, g.sm, H, (int)g.rows_alloc, s));
        HIP_TRY(launch_tokens(e->x, e->cls, e->pos_table, e->extra, g.nseq, g.sm, T, H, s, vl.row0));
        if (tokens_in)
            HIP_TRY(launch_embed_rows(c.in, nimg, N1, e->row_map, e->pidx, e->sidx, e->pos_table, use_scales ? e->scale_table : nullptr, e->x, H, s, R0));
    }
    if (!tokens_in) {
        Prof p(e, s, VTQ_K_PATCH);
        GemmArgs a = gemm_args(View{e->big, e->big_plane, (int)e->PDp}, e->patch, (int)g.P_pad, View{}, 1.0f / e->s_patch);
        a.x = e->x;
        a.row_map = e->row_map; a.idx1 = e->pidx; a.table1 = e->pos_table;
        a.idx2 = e->sidx; a.table2 = use_scales ? e->scale_table : nullptr;
        HIP_TRY(launch_gemm(a, e->lin, EPI_EMBED, s));
    }
    if (e->trace) HIP_TRY(launch_copy_tokens(e->x, e->trace, g.nseq, g.sm, T, H, s));

    // The last 64-key tile of the last sequence reads K / V rows up to 63 past M_pad in the QKV layout of `big`.  Masked keys
    // multiply by probability 0, which only holds for FINITE stale values: a previous forward that overflowed (inf / NaN, see
    // vtq_input_errors bit 1) with a larger batch would otherwise poison this one's first layer.  From layer 1 on the region
    // holds this forward's own fc1 output.  128 rows: geometry()'s slack, which covers the <= 127 rows behind the last sequence that
    // vtq_k_attention may load (the 4-wave kernel's unconditional Q loads; tests/test_gpu_footprint.py test_attention pins that none of
    // them reaches an output, for zeros and for NaNs alike).
    for (int pl = 0; pl < e->apl; ++pl)
        HIP_TRY(hipMemsetAsync((char*)e->big + ((size_t)pl * e->big_plane + (size_t)g.M_pad * 3 * H) * 2, 0, (size_t)128 * 3 * H * 2, s));
    // (a rollout call: the same rows of every retained QKV buffer -- no later stage of this forward writes them, and an earlier,
    // larger call may have.  g is this call's geometry, so a variable-length call clears behind ITS M_pad)
    if (rollout)
        for (void* q : e->ro_qkv)
            for (int pl = 0; pl < e->apl; ++pl)
                HIP_TRY(hipMemsetAsync((char*)q + ((size_t)pl * e->ro_plane + (size_t)g.M_pad * 3 * H) * 2, 0, (size_t)128 * 3 * H * 2, s));

    // ---- encoder (transformer.py:363-378, 275-285) -------------------------------------------------------------
    // the trace tap needs every token row of the last layer (the CLS-only tail itself takes any sequence length)
    // (fp8 mode runs the full last layer: its CLS row then goes through the same e4m3 GEMMs as every other row)
    // (forward_vit needs every row of the last layer: always the full last layer)
    // (vtq_encode_reference / vtq_forward_cached encode single images in the form vtq_forward would pick: their rows meet in one difference)
    // (the variable-length entries refuse a trace and the fp8 engine before they get here: for them this is cls_prune && no adapters)
    const bool prune = e->cls_prune && !e->trace && !e->fp8 && cfg.num_adapters == 0 && (nimg > 1 || mode != REF_PAIRS);
    if (run_encoder(e, c, g, s, prune, vl)) return 1;
    return finish(e, c, g, s, prune, vl);
}

// What stands between a scoring entry and forward(): every refusal, stated once.  Which of them apply is read off the Call; the order is
//   1. the batch description (it needs no handle): a NULL count array, a NULL ref_index, the extents, a count < 1, a ref_index out of range,
//      a rollout asked for with a NULL rollout_out
//   2. the handle: NULL, the fp8 experiment's engine, a set token trace
//   3. a NULL tensor, a NULL output
//   4. rollout calls: vtq_debug_stop_after, the sequence cap (the combine launch's grid)
//   5. variable-length calls: the sums and the maximum of the counts, the kernels' 32-bit row index
//   6. the scale rule, the weights -- then forward()
static int submit(vtq_handle e, Call c, void* stream) {
    const char* who = c.who;
    const int mode = c.rg.mode, B = c.B, G = c.rg.G, N = c.N;
    const bool pairs = mode == REF_PAIRS, group = mode == REF_GROUP, indexed = group || mode == REF_CACHED;
    const int B0 = group ? G : B, M = mode == REF_ENCODE ? 1 : B, lists = group ? 2 : 1;       // vtq_forward_varlen: ONE count array
    const char* const counts[2] = {group ? "n_ref" : "n_patches", "n_dist"};
    // ---- 1
    for (int k = 0; c.varlen && k < lists; ++k)
        if (!c.n_img[k]) return fail("%s: null %s", who, counts[k]);
    if (indexed && !c.rg.ref_index) return fail("%s: null ref_index", who);
    if (pairs && (B < 1 || (!c.varlen && N < 1))) return c.varlen ? fail("%s: B=%d", who, B) : fail("%s: B=%d N=%d", who, B, N);
    if (!pairs && (G < 1 || M < 1 || (!c.varlen && N < 1)))
        return c.varlen ? fail("%s: G=%d M=%d", who, G, M) : fail("%s: G=%d M=%d N=%d", who, G, M, N);
    for (int k = 0; c.varlen && k < lists; ++k)
        for (int i = 0, n = k == 0 ? B0 : B; i < n; ++i)
            if (c.n_img[k][i] < 1)
                return fail("%s: %s[%d] = %d (every %s needs at least one patch)", who, counts[k], i, (int)c.n_img[k][i], pairs ? "pair" : "image");
    for (int m = 0; indexed && m < B; ++m)
        if (c.rg.ref_index[m] < 0 || c.rg.ref_index[m] >= G) return fail("%s: ref_index[%d] = %d outside [0, %d)", who, m, (int)c.rg.ref_index[m], G);
    if (c.rollout && !c.rollout_out) return fail("%s: null rollout_out", who);
    // ---- 2.  The fp8 experiment scores (ref, dist) pairs and triplets of patches, nothing else
    if (!e) return null_handle(who);
    if (e->fp8 && (!pairs || c.nimg == 1 || c.varlen || c.rollout)) return fail("%s: not available for the fp8 experiment's engine", who);
    if (e->fp8 && c.tokens_in) return fail("%s: the fp8 experiment has no pre-embedded input path", who);
    if (e->trace && (c.rollout || c.varlen || !pairs))
        return fail("%s: a token trace buffer is set (vtq_set_token_trace): %s", who, !pairs ? "the trace layout is per batch of pairs"
                    : c.varlen ? "the trace layout is per uniform batch" : "the trace tap runs the last layer in another form");
    // ---- 3
    const bool vit = pairs && c.nimg == 1;
    if (c.null_arrays) return fail("%s: null argument", who);
    for (int k = 0; k < c.nimg; ++k)
        if (!c.in[k] || !c.pos[k]) return fail(vit ? "%s: null input" : "%s: null tensor", who);
    if (mode == REF_CACHED && !c.rg.rows) return fail("%s: null tensor", who);
    if (!(vit ? c.out : mode == REF_ENCODE ? c.rg.rows : c.q_out)) return fail("%s: null output", who);
    // ---- 4
    const int64_t nseq = B0 + (int64_t)(c.nimg - 1) * B;
    if (c.rollout && e->dbg_stop >= 0) return fail("%s: vtq_debug_stop_after is set", who);
    if (c.rollout && nseq > 65535) return fail("%s: %lld sequences (a rollout call takes at most 65535)", who, (long long)nseq);
    // ---- 5
    if (c.varlen) {
        for (int k = 0; k < c.nimg; ++k)
            for (int i = 0, n = k == 0 ? B0 : B; i < n; ++i) {
                c.sumN[k] += c.n_img[k][i];
                if (c.n_img[k][i] > c.maxN) c.maxN = c.n_img[k][i];
            }
        const int64_t rows = c.sumN[0] + c.sumN[1] + nseq * e->T;
        if (rows + 512 > INT32_MAX / 4 || nseq * (c.maxN + e->T) + 512 > INT32_MAX / 4)
            return fail("%s: %lld token rows exceed the 32-bit row index of the kernels", who, (long long)rows);
    }
    // ---- 6
    if (e->cfg.num_scales > 1)
        for (int k = 0; k < c.nimg; ++k)
            if (!c.scales[k]) return fail("Model uses scale embedding but scales is passed as None.");   // transformer.py:547-548
    if (all_loaded(e, who)) return 1;
    return forward(e, c, stream);
}

// one image per item, the (ref, dist) pair, the (ref, dist1, dist2) triplet as a Call
static Call call_images(const char* who, bool tokens_in, int nimg, const float* const* in, const float* const* pos, const float* const* scales,
                        int32_t B, int32_t N, float* q_out) {
    Call c;
    c.who = who; c.tokens_in = tokens_in; c.nimg = nimg; c.B = B; c.N = N; c.q_out = q_out;
    for (int k = 0; k < nimg; ++k) { c.in[k] = in[k]; c.pos[k] = pos[k]; c.scales[k] = scales ? scales[k] : nullptr; }
    return c;
}
static Call call_single(const char* who, int32_t tokens_in, const float* in, const float* pos, const float* scales, int32_t B, int32_t N, float* q_out) {
    return call_images(who, tokens_in != 0, 1, &in, &pos, &scales, B, N, q_out);
}
static Call call_pair(const char* who, bool tokens_in, const float* in_ref, const float* in_dist, const float* pos_ref, const float* pos_dist,
                      const float* scales_ref, const float* scales_dist, int32_t B, int32_t N, float* q_out) {
    const float *in[2] = {in_ref, in_dist}, *pos[2] = {pos_ref, pos_dist}, *scales[2] = {scales_ref, scales_dist};
    return call_images(who, tokens_in, 2, in, pos, scales, B, N, q_out);
}

#ifdef VTQ_WITH_FP8
int vtq_fp8_calibrate(vtq_handle e, const float* patches_ref, const float* patches_dist, const float* pos_ref, const float* pos_dist,
                      const float* scales_ref, const float* scales_dist, int32_t B, int32_t N, float* q_out, void* stream) {
    if (!e || !e->fp8) return fail("vtq_fp8_calibrate: not an fp8 engine");
    e->fp8_calibrated = false;
    e->fp8_installed = false;
    const bool was_static = e->fp8_static;
    e->fp8_static = false;
    const int rc = vtq_forward(e, patches_ref, patches_dist, pos_ref, pos_dist, scales_ref, scales_dist, B, N, q_out, stream);
    e->fp8_static = was_static;
    return rc;
}

int vtq_fp8_get_scales(vtq_handle e, float* out, int32_t cap) {
    if (!e || !e->fp8) return -1;
    const int L = e->cfg.num_layers, n = 1 + 4 * L;
    if (out) {
        std::vector<float> v(n);
        v[0] = e->s_patch;
        for (int i = 0; i < L; ++i) { v[1 + 4 * i] = e->s_ln1[i]; v[2 + 4 * i] = e->s_att[i]; v[3 + 4 * i] = e->s_ln2[i]; v[4 + 4 * i] = e->s_gelu[i]; }
        for (int i = 0; i < n && i < cap; ++i) out[i] = v[i];
    }
    return n;
}

int vtq_fp8_set_scales(vtq_handle e, const float* in, int32_t n) {
    if (!e || !e->fp8 || !in) return fail("vtq_fp8_set_scales: not an fp8 engine / null argument");
    const int L = e->cfg.num_layers;
    if (n != 1 + 4 * L) return fail("vtq_fp8_set_scales: %d values, expected %d (patches, then LN1 / attention / LN2 / GELU per layer)", n, 1 + 4 * L);
    for (int i = 0; i < n; ++i) {
        int ex = 0;
        if (!(in[i] > 0.0f) || !std::isfinite(in[i]) || frexpf(in[i], &ex) != 0.5f) return fail("vtq_fp8_set_scales: scale %d = %g is not a positive power of two", i, in[i]);
    }
    e->s_patch = in[0];
    for (int i = 0; i < L; ++i) { e->s_ln1[i] = in[1 + 4 * i]; e->s_att[i] = in[2 + 4 * i]; e->s_ln2[i] = in[3 + 4 * i]; e->s_gelu[i] = in[4 + 4 * i]; }
    e->fp8_calibrated = true;
    e->fp8_installed = true;
    return 0;
}

int vtq_fp8_reset(vtq_handle e) {
    if (!e || !e->fp8) return fail("vtq_fp8_reset: not an fp8 engine");
    e->fp8_calibrated = false;                 // the next forward calibrates on its own batch again
    e->fp8_installed = false;
    return 0;
}
#endif

// ---- the scoring entries (include/vtamiq_hip.h): each describes its request as a Call -- the constructors above and below, plus the few
// fields that differ -- and hands it to submit()
static Call call_triplet(const char* who, bool tokens_in, const float* const* in, const float* const* pos, const float* const* scales, int32_t B,
                         int32_t N, float* q_out) {
    static const float* const none[3] = {};
    Call c = call_images(who, tokens_in, 3, in ? in : none, pos ? pos : none, scales, B, N, q_out);
    c.null_arrays = !in || !pos;
    return c;
}
// one-to-many scoring, every reference encoded once: G references + M distorted images in one batch; G references alone, their rows to the
// caller's cache; M distorted images against the cached rows
static Call call_group(const char* who, bool tokens_in, const float* in_ref, const float* in_dist, const float* pos_ref, const float* pos_dist,
                       const float* scales_ref, const float* scales_dist, int32_t G, int32_t M, int32_t N, const int32_t* ref_index, float* q_out) {
    Call c = call_pair(who, tokens_in, in_ref, in_dist, pos_ref, pos_dist, scales_ref, scales_dist, M, N, q_out);
    c.rg = RefGroup{REF_GROUP, G, ref_index, nullptr};
    return c;
}
static Call call_encode(const char* who, int32_t tokens_in, const float* in, const float* pos, const float* scales, int32_t G, int32_t N,
                        float* ref_rows) {
    Call c = call_single(who, tokens_in, in, pos, scales, G, N, nullptr);
    c.rg = RefGroup{REF_ENCODE, G, nullptr, ref_rows};
    return c;
}
static Call call_cached(const char* who, const float* ref_rows, int32_t G, int32_t tokens_in, const float* in, const float* pos,
                        const float* scales, int32_t M, int32_t N, const int32_t* ref_index, float* q_out) {
    Call c = call_single(who, tokens_in, in, pos, scales, M, N, q_out);
    c.rg = RefGroup{REF_CACHED, G, ref_index, const_cast<float*>(ref_rows)};
    return c;
}
// Images of different patch counts: host count arrays in place of N.  Sequences are packed back to back at their own length, image 0's, then
// image 1's, the packed patch rows likewise (image, item, patch).  Every kernel is row- or sequence-independent and the GEMMs are bitwise
// independent of M, so a sequence has the bits of the uniform entry on that item alone.
static Call with_counts(Call c, const int32_t* n0, const int32_t* n1) {
    c.varlen = true; c.n_img[0] = n0; c.n_img[1] = n1;
    return c;
}
// The rollout forms: the maps of every sequence the call encodes, in call order (image 0's, then image 1's); last_attention_out may be NULL
static Call with_rollout(Call c, float* rollout_out, float* last_attention_out) {
    c.rollout = true; c.rollout_out = rollout_out; c.last_attention_out = last_attention_out;
    return c;
}

int vtq_forward(vtq_handle e, const float* patches_ref, const float* patches_dist, const float* pos_ref, const float* pos_dist,
                const float* scales_ref, const float* scales_dist, int32_t B, int32_t N, float* q_out, void* stream) {
    return submit(e, call_pair("vtq_forward", false, patches_ref, patches_dist, pos_ref, pos_dist, scales_ref, scales_dist, B, N, q_out), stream);
}

int vtq_forward_tokens(vtq_handle e, const float* feats_ref, const float* feats_dist, const float* pos_ref, const float* pos_dist,
                       const float* scales_ref, const float* scales_dist, int32_t B, int32_t N, float* q_out, void* stream) {
    return submit(e, call_pair("vtq_forward_tokens", true, feats_ref, feats_dist, pos_ref, pos_dist, scales_ref, scales_dist, B, N, q_out), stream);
}

int vtq_forward_rollout(vtq_handle e, const float* patches_ref, const float* patches_dist, const float* pos_ref, const float* pos_dist,
                        const float* scales_ref, const float* scales_dist, int32_t B, int32_t N, float* q_out, float* rollout_out,
                        float* last_attention_out, void* stream) {
    return submit(e, with_rollout(call_pair("vtq_forward_rollout", false, patches_ref, patches_dist, pos_ref, pos_dist, scales_ref, scales_dist, B, N,
                                            q_out), rollout_out, last_attention_out), stream);
}

int vtq_forward_rollout_tokens(vtq_handle e, const float* feats_ref, const float* feats_dist, const float* pos_ref, const float* pos_dist,
                               const float* scales_ref, const float* scales_dist, int32_t B, int32_t N, float* q_out, float* rollout_out,
                               float* last_attention_out, void* stream) {
    return submit(e, with_rollout(call_pair("vtq_forward_rollout_tokens", true, feats_ref, feats_dist, pos_ref, pos_dist, scales_ref, scales_dist, B,
                                            N, q_out), rollout_out, last_attention_out), stream);
}

size_t vtq_rollout_workspace_bytes(vtq_handle e, int32_t B, int32_t N) { return (e && B >= 1 && N >= 1) ? ws_bytes(rollout_workspace(e, B, N)) : 0; }

int vtq_forward_varlen(vtq_handle e, const float* patches_ref, const float* patches_dist, const float* pos_ref, const float* pos_dist,
                       const float* scales_ref, const float* scales_dist, int32_t B, const int32_t* n_patches, float* q_out, void* stream) {
    return submit(e, with_counts(call_pair("vtq_forward_varlen", false, patches_ref, patches_dist, pos_ref, pos_dist, scales_ref, scales_dist, B, 0,
                                           q_out), n_patches, n_patches), stream);
}

int vtq_forward_varlen_rollout(vtq_handle e, const float* patches_ref, const float* patches_dist, const float* pos_ref, const float* pos_dist,
                               const float* scales_ref, const float* scales_dist, int32_t B, const int32_t* n_patches, float* q_out,
                               float* rollout_out, float* last_attention_out, void* stream) {
    return submit(e, with_rollout(with_counts(call_pair("vtq_forward_varlen_rollout", false, patches_ref, patches_dist, pos_ref, pos_dist, scales_ref,
                                                        scales_dist, B, 0, q_out), n_patches, n_patches), rollout_out, last_attention_out), stream);
}

int vtq_forward_pairwise(vtq_handle e, const float* const* patches, const float* const* pos, const float* const* scales, int32_t B,
                         int32_t N, float* q_out, void* stream) {
    return submit(e, call_triplet("vtq_forward_pairwise", false, patches, pos, scales, B, N, q_out), stream);
}

int vtq_forward_pairwise_tokens(vtq_handle e, const float* const* feats, const float* const* pos, const float* const* scales, int32_t B,
                                int32_t N, float* q_out, void* stream) {
    return submit(e, call_triplet("vtq_forward_pairwise_tokens", true, feats, pos, scales, B, N, q_out), stream);
}

int vtq_forward_vit(vtq_handle e, const float* in, int32_t tokens_in, const float* pos, const float* scales, int32_t B, int32_t N,
                    int32_t all_tokens, float* out, float* states, float* probs, void* stream) {
    Call c = call_single("vtq_forward_vit", tokens_in, in, pos, scales, B, N, nullptr);
    c.out = out;
    c.states = states;
    c.probs = probs;
    c.rows = e ? (all_tokens ? N + e->T : e->T) : 0;          // (a NULL handle is refused by submit())
    return submit(e, c, stream);
}

int vtq_forward_group(vtq_handle e, const float* patches_ref, const float* patches_dist, const float* pos_ref, const float* pos_dist,
                      const float* scales_ref, const float* scales_dist, int32_t G, int32_t M, int32_t N, const int32_t* ref_index,
                      float* q_out, void* stream) {
    return submit(e, call_group("vtq_forward_group", false, patches_ref, patches_dist, pos_ref, pos_dist, scales_ref, scales_dist, G, M, N, ref_index,
                                q_out), stream);
}

int vtq_forward_group_tokens(vtq_handle e, const float* feats_ref, const float* feats_dist, const float* pos_ref, const float* pos_dist,
                             const float* scales_ref, const float* scales_dist, int32_t G, int32_t M, int32_t N, const int32_t* ref_index,
                             float* q_out, void* stream) {
    return submit(e, call_group("vtq_forward_group_tokens", true, feats_ref, feats_dist, pos_ref, pos_dist, scales_ref, scales_dist, G, M, N, ref_index,
                                q_out), stream);
}

int vtq_forward_group_rollout(vtq_handle e, const float* patches_ref, const float* patches_dist, const float* pos_ref, const float* pos_dist,
                              const float* scales_ref, const float* scales_dist, int32_t G, int32_t M, int32_t N, const int32_t* ref_index,
                              float* q_out, float* rollout_out, float* last_attention_out, void* stream) {
    return submit(e, with_rollout(call_group("vtq_forward_group_rollout", false, patches_ref, patches_dist, pos_ref, pos_dist, scales_ref, scales_dist,
                                             G, M, N, ref_index, q_out), rollout_out, last_attention_out), stream);
}

int vtq_forward_group_rollout_tokens(vtq_handle e, const float* feats_ref, const float* feats_dist, const float* pos_ref, const float* pos_dist,
                                     const float* scales_ref, const float* scales_dist, int32_t G, int32_t M, int32_t N, const int32_t* ref_index,
                                     float* q_out, float* rollout_out, float* last_attention_out, void* stream) {
    return submit(e, with_rollout(call_group("vtq_forward_group_rollout_tokens", true, feats_ref, feats_dist, pos_ref, pos_dist, scales_ref, scales_dist,
                                             G, M, N, ref_index, q_out), rollout_out, last_attention_out), stream);
}

int vtq_encode_reference(vtq_handle e, const float* in, int32_t tokens_in, const float* pos, const float* scales, int32_t G, int32_t N,
                         float* ref_rows, void* stream) {
    return submit(e, call_encode("vtq_encode_reference", tokens_in, in, pos, scales, G, N, ref_rows), stream);
}

int vtq_encode_reference_rollout(vtq_handle e, const float* in, int32_t tokens_in, const float* pos, const float* scales, int32_t G, int32_t N,
                                 float* ref_rows, float* rollout_out, float* last_attention_out, void* stream) {
    return submit(e, with_rollout(call_encode("vtq_encode_reference_rollout", tokens_in, in, pos, scales, G, N, ref_rows), rollout_out,
                                  last_attention_out), stream);
}

int vtq_forward_cached(vtq_handle e, const float* ref_rows, int32_t G, const float* in, int32_t tokens_in, const float* pos, const float* scales,
                       int32_t M, int32_t N, const int32_t* ref_index, float* q_out, void* stream) {
    return submit(e, call_cached("vtq_forward_cached", ref_rows, G, tokens_in, in, pos, scales, M, N, ref_index, q_out), stream);
}

// the M distorted sequences' maps only: the cached references' come from vtq_encode_reference_rollout
int vtq_forward_cached_rollout(vtq_handle e, const float* ref_rows, int32_t G, const float* in, int32_t tokens_in, const float* pos,
                               const float* scales, int32_t M, int32_t N, const int32_t* ref_index, float* q_out, float* rollout_out,
                               float* last_attention_out, void* stream) {
    return submit(e, with_rollout(call_cached("vtq_forward_cached_rollout", ref_rows, G, tokens_in, in, pos, scales, M, N, ref_index, q_out),
                                  rollout_out, last_attention_out), stream);
}

int vtq_forward_group_varlen(vtq_handle e, const float* patches_ref, const float* patches_dist, const float* pos_ref, const float* pos_dist,
                             const float* scales_ref, const float* scales_dist, int32_t G, int32_t M, const int32_t* n_ref, const int32_t* n_dist,
                             const int32_t* ref_index, float* q_out, void* stream) {
    return submit(e, with_counts(call_group("vtq_forward_group_varlen", false, patches_ref, patches_dist, pos_ref, pos_dist, scales_ref, scales_dist, G,
                                            M, 0, ref_index, q_out), n_ref, n_dist), stream);
}

int vtq_forward_group_varlen_rollout(vtq_handle e, const float* patches_ref, const float* patches_dist, const float* pos_ref, const float* pos_dist,
                                     const float* scales_ref, const float* scales_dist, int32_t G, int32_t M, const int32_t* n_ref,
                                     const int32_t* n_dist, const int32_t* ref_index, float* q_out, float* rollout_out, float* last_attention_out,
                                     void* stream) {
    return submit(e, with_rollout(with_counts(call_group("vtq_forward_group_varlen_rollout", false, patches_ref, patches_dist, pos_ref, pos_dist,
                                                         scales_ref, scales_dist, G, M, 0, ref_index, q_out), n_ref, n_dist),
                                  rollout_out, last_attention_out), stream);
}

int vtq_encode_reference_varlen(vtq_handle e, const float* patches, const float* pos, const float* scales, int32_t G, const int32_t* n_patches,
                                float* ref_rows, void* stream) {
    return submit(e, with_counts(call_encode("vtq_encode_reference_varlen", 0, patches, pos, scales, G, 0, ref_rows), n_patches, nullptr), stream);
}

int vtq_encode_reference_varlen_rollout(vtq_handle e, const float* patches, const float* pos, const float* scales, int32_t G,
                                        const int32_t* n_patches, float* ref_rows, float* rollout_out, float* last_attention_out, void* stream) {
    return submit(e, with_rollout(with_counts(call_encode("vtq_encode_reference_varlen_rollout", 0, patches, pos, scales, G, 0, ref_rows), n_patches,
                                              nullptr), rollout_out, last_attention_out), stream);
}

int vtq_forward_cached_varlen(vtq_handle e, const float* ref_rows, int32_t G, const float* patches, const float* pos, const float* scales, int32_t M,
                              const int32_t* n_patches, const int32_t* ref_index, float* q_out, void* stream) {
    return submit(e, with_counts(call_cached("vtq_forward_cached_varlen", ref_rows, G, 0, patches, pos, scales, M, 0, ref_index, q_out), n_patches,
                                 nullptr), stream);
}

int vtq_forward_cached_varlen_rollout(vtq_handle e, const float* ref_rows, int32_t G, const float* patches, const float* pos, const float* scales,
                                      int32_t M, const int32_t* n_patches, const int32_t* ref_index, float* q_out, float* rollout_out,
                                      float* last_attention_out, void* stream) {
    return submit(e, with_rollout(with_counts(call_cached("vtq_forward_cached_varlen_rollout", ref_rows, G, 0, patches, pos, scales, M, 0, ref_index,
                                                          q_out), n_patches, nullptr), rollout_out, last_attention_out), stream);
}

int vtq_input_errors(vtq_handle e, int32_t* flags, void* stream) {
    if (!e || !flags) return fail("vtq_input_errors: null argument");
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(e->err_host, e->err_flag, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *flags = *e->err_host;
    HIP_TRY(hipMemsetAsync(e->err_flag, 0, 4, s));      // after the wait: it runs under the caller's next host-side work, ahead of the next forward in stream order
    return 0;
}

// ---- per-kernel entry points -------------------------------------------------------------------------------------
int vtq_k_split(const float* src, void* dst, int64_t plane_stride, int64_t numel, int32_t f16, int32_t planes, void* stream) {
    HIP_TRY(launch_split(src, dst, plane_stride, numel, f16, planes, (hipStream_t)stream));
    return 0;
}

int vtq_k_gemm_schedule(int32_t M, int32_t N, int32_t K, int32_t wplanes, int32_t* out, int32_t cap) {
    if (M < 256 || N < 256 || M % 256 || N % 256 || K < 1 || wplanes < 1 || wplanes > 2) return -1;
    const std::vector<int> v = gemm_tile_schedule(M / 256, N / 256, K, wplanes);
    if (out)
        for (size_t i = 0; i < v.size() && (int32_t)i < cap; ++i) out[i] = v[i];
    return (int)v.size();
}

int vtq_k_gemm(const void* A, int64_t a_plane, int32_t lda, const void* W, int64_t w_plane, int32_t M, int32_t N, int32_t K,
               int32_t num, int32_t epilogue, const float* bias, const float* gamma, float* x_f32, void* out16,
               int64_t o_plane, int32_t ldo, void* stream) {
    if (epilogue < 0 || epilogue > 2) return fail("vtq_k_gemm: epilogue %d", epilogue);
    const Num nm = num_from_code(num);
    if (!num_valid(nm)) return fail("vtq_k_gemm: operand format code %d", num);
    GemmArgs a{};
    a.A = A; a.a_plane = a_plane; a.lda = lda; a.W = W; a.w_plane = w_plane; a.M = M; a.N = N; a.K = K;
    a.bias = bias; a.gamma = gamma; a.x = x_f32; a.out = out16; a.o_plane = o_plane; a.ldo = ldo;
    HIP_TRY(launch_gemm(a, nm, epilogue, (hipStream_t)stream));
    return 0;
}

int vtq_k_gemm_rowln(const void* A, int64_t a_plane, int32_t lda, const void* W, int64_t w_plane, int32_t M, int32_t K, int32_t num,
                     const float* bias, const float* gamma, float* x_f32, const float* ln_w, const float* ln_b, void* out16, int64_t o_plane,
                     void* stream) {
    const Num nm = num_from_code(num);
    if (!num_valid(nm) || nm.terms != 3) return fail("vtq_k_gemm_rowln: operand format code %d (3-term formats only)", num);
    RowLnArgs a{};
    a.A = A; a.a_plane = a_plane; a.lda = lda; a.W = W; a.w_plane = w_plane; a.M = M; a.N = 768; a.K = K; a.bias = bias; a.gamma = gamma;
    a.x = x_f32; a.ln_w = ln_w; a.ln_b = ln_b; a.out = out16; a.o_plane = o_plane;
    HIP_TRY(launch_gemm_rowln(a, nm, (hipStream_t)stream));
    return 0;
}

#ifdef VTQ_WITH_FP8
int vtq_k_quant_rows_fp8(const float* W, void* dst, float* inv_scale, int32_t N, int32_t K, void* stream) {
    if (!W || !dst || !inv_scale || N < 1 || K < 4) return fail("vtq_k_quant_rows_fp8: bad argument");
    HIP_TRY(launch_quant_rows_fp8(W, dst, inv_scale, N, K, (hipStream_t)stream));
    return 0;
}

int vtq_k_quant_fp8(const float* src, void* dst, int64_t numel, float scale, void* stream) {
    HIP_TRY(launch_split(src, dst, 0, numel, 2, 1, (hipStream_t)stream, scale));
    return 0;
}

int vtq_k_gemm_fp8(const void* A8, int32_t lda, const void* W8, const float* wscale, float ascale_inv, int32_t M, int32_t N, int32_t K,
                   int32_t epilogue, const float* bias, const float* gamma, float* x_f32, void* out, int64_t o_plane, int32_t ldo,
                   float out_scale, void* stream) {
    if (epilogue < 0 || epilogue > 2) return fail("vtq_k_gemm_fp8: epilogue %d", epilogue);
    GemmArgs a{};
    a.A = A8; a.lda = lda; a.W = W8; a.M = M; a.N = N; a.K = K; a.bias = bias; a.gamma = gamma; a.x = x_f32; a.out = out; a.o_plane = o_plane;
    a.ldo = ldo; a.wscale = wscale; a.ascale_inv = ascale_inv; a.out_scale = out_scale;
    HIP_TRY(launch_gemm(a, Num{2, 1}, epilogue, (hipStream_t)stream));
    return 0;
}
#endif

int vtq_k_layernorm(const float* x, const float* w, const float* b, void* out, int64_t o_plane, int32_t rows, int32_t H,
                    int32_t f16, int32_t planes, void* stream) {
    HIP_TRY(launch_layernorm(x, w, b, out, o_plane, rows, H, f16, planes, (hipStream_t)stream));
    return 0;
}

int vtq_k_attention(const void* qkv, int64_t plane, void* out, int64_t o_plane, int32_t nseq, int32_t S, int32_t S_pad,
                    int32_t H, int32_t num, void* stream) {
    const Num nm = num_from_code(num);
    if (!num_valid(nm) || nm.terms == 2) return fail("vtq_k_attention: operand format code %d", num);
    HIP_TRY(launch_attention(qkv, plane, out, o_plane, nseq, S, S_pad, H, nm, (hipStream_t)stream));
    return 0;
}

// the attention block table of nseq sequences (4 ints per workgroup), or an empty one for what vtq_vl_attention_blocks answers with -1
static std::vector<int> vl_blocks_checked(int32_t nseq, const int32_t* seq_len, int32_t H) {
    if (nseq < 1 || !seq_len || H < 64 || H % 64) return {};
    int64_t rows = 0;
    for (int j = 0; j < nseq; ++j) {
        if (seq_len[j] < 1) return {};
        rows += seq_len[j];
    }
    if (rows + 512 > INT32_MAX / 4) return {};
    return attention_varlen_blocks(seq_len, nseq, H);
}

int vtq_vl_attention_blocks(int32_t nseq, const int32_t* seq_len, int32_t H, int32_t* out, int32_t cap) {
    const std::vector<int> t = vl_blocks_checked(nseq, seq_len, H);
    if (t.empty()) return -1;
    if (out)
        for (size_t i = 0; i < t.size() && (int64_t)i < (int64_t)cap * 4; ++i) out[i] = t[i];
    return (int)(t.size() / 4);
}

int vtq_vl_attention(const void* qkv, int64_t plane, void* out, int64_t o_plane, int32_t nseq, const int32_t* seq_len, int32_t H, int32_t num,
                     void* stream) {
    const Num nm = num_from_code(num);
    if (!num_valid(nm) || nm.terms == 2 || nm.f16 > 1) return fail("vtq_vl_attention: operand format code %d", num);
    if (!qkv || !out || !seq_len) return fail("vtq_vl_attention: null argument");
    const std::vector<int> t = vl_blocks_checked(nseq, seq_len, H);
    const int nblocks = (int)(t.size() / 4);
    if (nblocks < 1) return fail("vtq_vl_attention: nseq=%d, H=%d or a sequence length < 1", (int)nseq, (int)H);
    hipStream_t s = (hipStream_t)stream;
    int* dev = nullptr;
    HIP_TRY(hipMalloc((void**)&dev, t.size() * sizeof(int)));
    hipError_t err = hipMemcpyAsync(dev, t.data(), t.size() * sizeof(int), hipMemcpyHostToDevice, s);
    if (err == hipSuccess) err = launch_attention_varlen(qkv, plane, out, o_plane, dev, nblocks, H, nm, s);
    const hipError_t err2 = hipStreamSynchronize(s);        // the table is a temporary of this call
    (void)hipFree(dev);
    if (err != hipSuccess || err2 != hipSuccess) return fail("vtq_vl_attention: %s", hipGetErrorString(err != hipSuccess ? err : err2));
    return 0;
}

int vtq_k_attention_probs(const void* qkv, int64_t plane, float* probs, int32_t nseq, int32_t S, int32_t S_pad, int32_t H, int32_t num,
                          int32_t q_log2, void* stream) {
    const Num nm = num_from_code(num);
    if (!num_valid(nm) || nm.terms == 2 || nm.f16 > 1) return fail("vtq_k_attention_probs: operand format code %d", num);
    if (!qkv || !probs || nseq < 1 || S < 1 || S_pad < S || H < 64 || H % 64) return fail("vtq_k_attention_probs: bad argument");
    if (q_log2 && nm.terms != 3) return fail("vtq_k_attention_probs: q_log2 applies to the 3-term formats only");
    HIP_TRY(launch_attention_probs(qkv, plane, probs, nseq, S, S_pad, H, nm, (hipStream_t)stream, q_log2 != 0));
    return 0;
}

int vtq_k_rollout_step(const void* qkv, int64_t plane, const float* r_in, float* r_out, float* part, int32_t nseq, int32_t S, int32_t S_pad,
                       int32_t H, int32_t num, int32_t q_log2, void* stream) {
    const Num nm = num_from_code(num);
    if (!num_valid(nm) || nm.terms == 2 || nm.f16 > 1) return fail("vtq_k_rollout_step: operand format code %d", num);
    if (!qkv || !r_in || !r_out || !part || nseq < 1 || nseq > 65535 || S < 1 || S_pad < S || H < 64 || H % 64) return fail("vtq_k_rollout_step: bad argument");
    if (q_log2 && nm.terms != 3) return fail("vtq_k_rollout_step: q_log2 applies to the 3-term formats only");
    HIP_TRY(launch_rollout_step(qkv, plane, r_in, 0, part, r_out, nullptr, nseq, S, S_pad, H, nm, (hipStream_t)stream, q_log2 != 0));
    return 0;
}

int vtq_vl_rollout_step(const void* qkv, int64_t plane, const float* r_in, float* r_out, float* part, int32_t nseq, const int32_t* seq_len,
                        int32_t H, int32_t num, int32_t q_log2, void* stream) {
    const Num nm = num_from_code(num);
    if (!num_valid(nm) || nm.terms == 2 || nm.f16 > 1) return fail("vtq_vl_rollout_step: operand format code %d", num);
    if (!qkv || !r_in || !r_out || !part || !seq_len) return fail("vtq_vl_rollout_step: null argument");
    if (q_log2 && nm.terms != 3) return fail("vtq_vl_rollout_step: q_log2 applies to the 3-term formats only");
    if (nseq > 65535) return fail("vtq_vl_rollout_step: nseq=%d (at most 65535)", (int)nseq);
    const std::vector<int> blocks = vl_blocks_checked(nseq, seq_len, H);
    const int nblocks = (int)(blocks.size() / 4);
    if (nblocks < 1) return fail("vtq_vl_rollout_step: nseq=%d, H=%d or a sequence length < 1", (int)nseq, (int)H);
    // the call's tables as forward() lays them out (Table): row offsets, lengths, then the block table
    const Table tb(nseq);
    std::vector<int> t((size_t)tb.blk + blocks.size(), 0);
    int64_t rows = 0;
    int smax = 0;
    for (int j = 0; j < nseq; ++j) {
        t[j] = (int)rows; t[tb.len + j] = seq_len[j];
        rows += seq_len[j];
        if (seq_len[j] > smax) smax = seq_len[j];
    }
    t[nseq] = (int)rows;
    memcpy(t.data() + tb.blk, blocks.data(), blocks.size() * sizeof(int));
    hipStream_t s = (hipStream_t)stream;
    int* dev = nullptr;
    HIP_TRY(hipMalloc((void**)&dev, t.size() * sizeof(int)));
    hipError_t err = hipMemcpyAsync(dev, t.data(), t.size() * sizeof(int), hipMemcpyHostToDevice, s);
    if (err == hipSuccess)
        err = launch_rollout_step_varlen(qkv, plane, r_in, 0, part, r_out, nullptr, dev + tb.blk, nblocks, dev, dev + tb.len, nseq, smax, rows, H, nm,
                                         s, q_log2 != 0);
    const hipError_t err2 = hipStreamSynchronize(s);        // the table is a temporary of this call
    (void)hipFree(dev);
    if (err != hipSuccess || err2 != hipSuccess) return fail("vtq_vl_rollout_step: %s", hipGetErrorString(err != hipSuccess ? err : err2));
    return 0;
}

int vtq_k_skinny_linear(const void* xa, int64_t xa_plane, int32_t ldx, const void* W, int64_t w_plane, int32_t R, int32_t N, int32_t K,
                        int32_t num, int32_t epi, const float* bias, const float* post_slope, const float* gamma, const float* res,
                        const float* aux, int32_t ldr, int32_t nsplit, float* y, int32_t ldy, int32_t ycols, void* ya, int64_t ya_plane,
                        int32_t ldya, int32_t pcol0, const float* next_slope, void* stream) {
    const Num nm = num_from_code(num);
    if (!num_valid(nm)) return fail("vtq_k_skinny_linear: operand format code %d", num);
    if (epi < SK_PLAIN || epi > SK_CONVCAT) return fail("vtq_k_skinny_linear: epilogue %d", epi);
    SkinnyArgs a{};
    a.xa = xa; a.xa_plane = xa_plane; a.ldx = ldx; a.W = W; a.w_plane = w_plane; a.R = R; a.N = N; a.K = K; a.bias = bias; a.epi = epi;
    a.post_slope = post_slope; a.gamma = gamma; a.res = res; a.aux = aux; a.ldr = ldr; a.nsplit = nsplit;
    a.y = y; a.ldy = ldy; a.ycols = ycols; a.ya = ya; a.ya_plane = ya_plane; a.ldya = ldya; a.ya_planes = nm.apl(); a.pcol0 = pcol0;
    a.next_slope = next_slope;
    HIP_TRY(launch_skinny(a, nm, (hipStream_t)stream));
    return 0;
}

int vtq_k_cls_fold_chunk_rows(void) { return cls_fold_chunk_rows(); }

int vtq_k_cls_fold(const float* q, const void* wqkv, int64_t w_plane, const float* bqkv, const float* x, int64_t seq_stride, const float* ln_w,
                   const float* ln_b, int32_t nseq, int32_t S, int32_t H, int32_t num, int32_t q_log2, float* u, float* part, void* z,
                   int64_t z_plane, float* ctx, void* stream) {
    const Num nm = num_from_code(num);
    if (!num_valid(nm) || nm.f16 > 1) return fail("vtq_k_cls_fold: operand format code %d", num);
    if (!q || !wqkv || !bqkv || !x || !ln_w || !ln_b || !u || !part || !z || !ctx || nseq < 1 || S < 1 || (H != 768 && H != 1024))
        return fail("vtq_k_cls_fold: bad argument");
    if (q_log2 && nm.terms != 3) return fail("vtq_k_cls_fold: q_log2 applies to the 3-term formats only");
    hipStream_t s = (hipStream_t)stream;
    const int nh = H / 64;
    const PlaneOut zo{z, z_plane, nh * H, nm.f16, nm.apl(), nullptr};
    HIP_TRY(launch_cls_fold(q, (const char*)wqkv + (size_t)H * H * 2, w_plane, H, nm.f16, nm.wpl(), x, seq_stride, ln_w, ln_b, u, part, nseq, S, H, zo, s,
                            q_log2 != 0));
    SkinnyArgs a{};
    a.xa = z; a.xa_plane = z_plane; a.ldx = nh * H; a.xcol64 = H; a.W = (const char*)wqkv + (size_t)2 * H * H * 2; a.w_plane = w_plane;
    a.R = nseq; a.N = H; a.K = H; a.bias = bqkv + 2 * H; a.epi = SK_PLAIN; a.y = ctx; a.ldy = H; a.ycols = H; a.ya_planes = nm.apl();
    HIP_TRY(launch_skinny(a, nm, s));
    return 0;
}

int vtq_vl_cls_fold(const float* q, const void* wqkv, int64_t w_plane, const float* bqkv, const float* x, const float* ln_w, const float* ln_b,
                    int32_t nseq, const int32_t* seq_len, int32_t H, int32_t num, int32_t q_log2, float* u, float* part, void* z, int64_t z_plane,
                    float* ctx, void* stream) {
    const Num nm = num_from_code(num);
    if (!num_valid(nm) || nm.f16 > 1) return fail("vtq_vl_cls_fold: operand format code %d", num);
    if (!q || !wqkv || !bqkv || !x || !ln_w || !ln_b || !seq_len || !u || !part || !z || !ctx) return fail("vtq_vl_cls_fold: null argument");
    if (nseq < 1 || nseq > 65535 || (H != 768 && H != 1024)) return fail("vtq_vl_cls_fold: nseq=%d, H=%d", (int)nseq, (int)H);
    if (q_log2 && nm.terms != 3) return fail("vtq_vl_cls_fold: q_log2 applies to the 3-term formats only");
    // the call's tables: row offsets [nseq], then lengths [nseq]
    std::vector<int> t((size_t)2 * nseq);
    int64_t rows = 0;
    int smax = 0;
    for (int j = 0; j < nseq; ++j) {
        if (seq_len[j] < 1) return fail("vtq_vl_cls_fold: sequence %d has length %d", j, (int)seq_len[j]);
        t[j] = (int)rows; t[nseq + j] = seq_len[j];
        rows += seq_len[j];
        if (seq_len[j] > smax) smax = seq_len[j];
        if (rows > INT32_MAX / 4) return fail("vtq_vl_cls_fold: more than %d rows", INT32_MAX / 4);
    }
    hipStream_t s = (hipStream_t)stream;
    const int nh = H / 64;
    int* dev = nullptr;
    HIP_TRY(hipMalloc((void**)&dev, t.size() * sizeof(int)));
    hipError_t err = hipMemcpyAsync(dev, t.data(), t.size() * sizeof(int), hipMemcpyHostToDevice, s);
    if (err == hipSuccess) {
        const PlaneOut zo{z, z_plane, nh * H, nm.f16, nm.apl(), nullptr};
        err = launch_cls_fold(q, (const char*)wqkv + (size_t)H * H * 2, w_plane, H, nm.f16, nm.wpl(), x, 0, ln_w, ln_b, u, part, nseq, smax, H, zo, s,
                              q_log2 != 0, VarSeq{dev, dev + nseq});
    }
    if (err == hipSuccess) {
        SkinnyArgs a{};
        a.xa = z; a.xa_plane = z_plane; a.ldx = nh * H; a.xcol64 = H; a.W = (const char*)wqkv + (size_t)2 * H * H * 2; a.w_plane = w_plane;
        a.R = nseq; a.N = H; a.K = H; a.bias = bqkv + 2 * H; a.epi = SK_PLAIN; a.y = ctx; a.ldy = H; a.ycols = H; a.ya_planes = nm.apl();
        err = launch_skinny(a, nm, s);
    }
    const hipError_t err2 = hipStreamSynchronize(s);        // the tables are temporaries of this call
    (void)hipFree(dev);
    if (err != hipSuccess || err2 != hipSuccess) return fail("vtq_vl_cls_fold: %s", hipGetErrorString(err != hipSuccess ? err : err2));
    return 0;
}

int vtq_k_diffnet_head(vtq_handle e, const float* d, int32_t HB, float* q_out, void* stream) {
    if (!e || !d || !q_out || HB < 1) return fail("vtq_k_diffnet_head: bad argument");
    if (all_loaded(e, "vtq_k_diffnet_head")) return 1;
    if (reserve(e, (HB + 1) / 2, 1)) return 1;
    return run_head(e, d, HB, q_out, (hipStream_t)stream);
}

int vtq_k_repeat_mean(const float* q, double* out, int32_t R, int32_t N, void* stream) {
    if (!q || !out || R < 1 || N < 1) return fail("vtq_k_repeat_mean: bad argument");
    HIP_TRY(launch_repeat_mean(q, out, R, N, (hipStream_t)stream));
    return 0;
}

int vtq_k_rank_metrics(const double* a, const double* b, int32_t N, int32_t normalize, double* work, int64_t* counts, double* out,
                       void* stream) {
    if (!a || !b || !work || !counts || !out || N < 2) return fail("vtq_k_rank_metrics: bad argument");
    HIP_TRY(launch_rank_metrics(a, b, N, normalize, work, work + N, work + 2 * (int64_t)N, work + 3 * (int64_t)N, (long long*)counts, out,
                                (hipStream_t)stream));
    return 0;
}

int vtq_k_image_normalize(const uint8_t* images, float* out, int32_t NI, int32_t H, int32_t W, const int32_t* flips, const float* mean,
                          const float* std_, void* stream) {
    if (!images || !out || !mean || !std_ || NI < 1 || H < 1 || W < 1) return fail("vtq_k_image_normalize: bad argument");
    HIP_TRY(launch_image_normalize(images, out, NI, H, W, flips, mean, std_, (hipStream_t)stream));
    return 0;
}

int vtq_k_avgpool2(const float* in, float* out, int32_t NC, int32_t H, int32_t W, void* stream) {
    HIP_TRY(launch_avgpool2(in, out, NC, H, W, (hipStream_t)stream));
    return 0;
}

int vtq_k_gather_patches(const float* const* levels, const int32_t* hs, const int32_t* ws, int32_t nlevels, const int32_t* samples,
                         const int32_t* scale_ids, float* patches, float* pos, float* scales, int32_t NI, int32_t N, int32_t patch_size,
                         void* stream) {
    if (!levels || !hs || !ws || !samples || !patches || !pos) return fail("vtq_k_gather_patches: null argument");
    if (patch_size != 16 && patch_size != 8) return fail("vtq_k_gather_patches: patch_size %d (16 or 8)", patch_size);
    HIP_TRY(launch_gather_patches(levels, hs, ws, nlevels, samples, scale_ids, patches, pos, scales, NI, N, (hipStream_t)stream, patch_size));
    return 0;
}

// include/vtamiq_hip_images.h, include/vtamiq_hip_tensors.h: the checks the two gathers share, stated once.  Every check reads HOST arrays
// only, so a refusal touches no device memory and launches nothing.  elem: bytes per pixel element (1 for the uint8 HWC images)
static int gather_refused(const char* name, int64_t elem, const void* images, int64_t image_bytes, const int32_t* tab, const int32_t* patch_img,
                          const int64_t* img_off, const int32_t* H, const int32_t* W, const int32_t* row0, int32_t NI, const int32_t* samples,
                          const int32_t* scale_ids, const float* mean, const float* std_, const float* patches, const float* pos,
                          int32_t patch_size, int32_t num_scales) {
    if (!images || !tab || !patch_img || !img_off || !H || !W || !row0 || !samples || !mean || !std_ || !patches || !pos)
        return fail("%s: null argument", name);
    if ((uintptr_t)tab % 16) return fail("%s: tab is not 16-byte aligned", name);
    if (NI < 1) return fail("%s: NI=%d (at least 1)", name, (int)NI);
    if (patch_size != 16 && patch_size != 8) return fail("%s: patch_size %d (16 or 8)", name, (int)patch_size);
    if (num_scales < 1 || num_scales > 4) return fail("%s: num_scales=%d (1 .. 4)", name, (int)num_scales);
    if (!scale_ids && num_scales > 1) return fail("%s: scale_ids are required when num_scales > 1", name);
    if (row0[0] != 0) return fail("%s: row0[0]=%d (0 required)", name, (int)row0[0]);
    for (int32_t i = 0; i < NI; ++i) {
        if (row0[i + 1] < row0[i]) return fail("%s: row0 decreases at image %d", name, (int)i);
        if (H[i] < patch_size || W[i] < patch_size)
            return fail("%s: image %d (%d x %d) is smaller than one %d x %d patch", name, (int)i, (int)H[i], (int)W[i], (int)patch_size,
                        (int)patch_size);
        if (img_off[i] % elem)
            return fail("%s: image %d starts at byte %lld, not a multiple of the element size %d", name, (int)i, (long long)img_off[i], (int)elem);
        if (img_off[i] < 0 || image_bytes < 0 || img_off[i] > image_bytes || (int64_t)3 * H[i] * W[i] > (image_bytes - img_off[i]) / elem)
            return fail("%s: image %d (%d x %d at byte %lld) leaves the buffer of %lld bytes", name, (int)i, (int)H[i], (int)W[i],
                        (long long)img_off[i], (long long)image_bytes);
    }
    if (row0[NI] < 1) return fail("%s: no patches (row0[NI]=%d)", name, (int)row0[NI]);
    return 0;
}

int vtq_k_gather_patches_u8(const uint8_t* images, int64_t image_bytes, const int32_t* tab, const int32_t* patch_img, const int64_t* img_off,
                            const int32_t* H, const int32_t* W, const int32_t* row0, int32_t NI, const int32_t* samples,
                            const int32_t* scale_ids, const int32_t* flips, const float* mean, const float* std_, float* patches, float* pos,
                            float* scales, int32_t patch_size, int32_t num_scales, void* stream) {
    if (gather_refused("vtq_k_gather_patches_u8", 1, images, image_bytes, tab, patch_img, img_off, H, W, row0, NI, samples, scale_ids, mean, std_,
                       patches, pos, patch_size, num_scales))
        return 1;
    HIP_TRY(launch_gather_patches_u8(images, tab, patch_img, samples, scale_ids, flips, patches, pos, scales, row0[NI], mean, std_, patch_size,
                                     num_scales, (hipStream_t)stream));
    return 0;
}

int vtq_k_gather_patches_planar(const void* images, int64_t image_bytes, int32_t dtype, const int32_t* tab, const int32_t* patch_img,
                                const int64_t* img_off, const int32_t* H, const int32_t* W, const int32_t* row0, int32_t NI,
                                const int32_t* samples, const int32_t* scale_ids, const int32_t* flips, const float* mean, const float* std_,
                                float* patches, float* pos, float* scales, int32_t patch_size, int32_t num_scales, void* stream) {
    if (dtype != VTQ_PIXEL_F32 && dtype != VTQ_PIXEL_F16 && dtype != VTQ_PIXEL_BF16)
        return fail("vtq_k_gather_patches_planar: dtype %d (0 fp32, 1 fp16, 2 bf16)", (int)dtype);
    if (gather_refused("vtq_k_gather_patches_planar", dtype == VTQ_PIXEL_F32 ? 4 : 2, images, image_bytes, tab, patch_img, img_off, H, W, row0, NI,
                       samples, scale_ids, mean, std_, patches, pos, patch_size, num_scales))
        return 1;
    HIP_TRY(launch_gather_patches_planar(images, dtype, tab, patch_img, samples, scale_ids, flips, patches, pos, scales, row0[NI], mean, std_,
                                         patch_size, num_scales, (hipStream_t)stream));
    return 0;
}

// include/vtamiq_hip_sampler.h: like the gather above, every check reads HOST arrays only
int vtq_k_sample_grid(const int32_t* seg, const uint64_t* keys, const int32_t* seg_host, const uint64_t* keys_host, int32_t NS, uint64_t seed,
                      int32_t amount_q, int32_t* samples, int32_t* scale_ids, void* stream) {
    if (!seg || !keys || !seg_host || !keys_host || !samples) return fail("vtq_k_sample_grid: null argument");
    if ((uintptr_t)seg % 16) return fail("vtq_k_sample_grid: seg is not 16-byte aligned");
    if (NS < 1) return fail("vtq_k_sample_grid: NS=%d (at least 1)", (int)NS);
    if (amount_q < 0 || amount_q > 65535) return fail("vtq_k_sample_grid: amount_q=%d (0 .. 65535)", (int)amount_q);
    int64_t total = 0;
    int max_cells = 0;
    for (int32_t j = 0; j < NS; ++j) {
        const int32_t* t = seg_host + (int64_t)j * 8;
        const int32_t first = t[0], n = t[1], Hg = t[2], Wg = t[3], hm = t[4], wm = t[5], level = t[6];
        if (Hg < 1 || Wg < 1 || (int64_t)Hg * Wg > VTQ_SAMPLER_MAX_CELLS)
            return fail("vtq_k_sample_grid: segment %d has a grid of %d x %d cells (1 .. %d cells)", (int)j, (int)Hg, (int)Wg, VTQ_SAMPLER_MAX_CELLS);
        if (n < 1 || n > Hg * Wg) return fail("vtq_k_sample_grid: segment %d asks for %d samples of %d cells", (int)j, (int)n, (int)(Hg * Wg));
        if (hm < 0 || wm < 0 || hm >= VTQ_SAMPLER_MAX_EXTENT || wm >= VTQ_SAMPLER_MAX_EXTENT)
            return fail("vtq_k_sample_grid: segment %d has h - P = %d, w - P = %d (0 .. %d)", (int)j, (int)hm, (int)wm, VTQ_SAMPLER_MAX_EXTENT - 1);
        if (level < 0 || level > 3) return fail("vtq_k_sample_grid: segment %d is on level %d (0 .. 3)", (int)j, (int)level);
        if (level != 0 && !scale_ids) return fail("vtq_k_sample_grid: scale_ids are required when a segment is on level %d", (int)level);
        if (first != total) return fail("vtq_k_sample_grid: segment %d starts at row %d, the segments before it end at %lld", (int)j, (int)first, (long long)total);
        total += n;
        if (total > 0x7fffffff) return fail("vtq_k_sample_grid: more than 2^31 - 1 samples");
        max_cells = Hg * Wg > max_cells ? Hg * Wg : max_cells;
    }
    HIP_TRY(launch_sample_grid(seg, keys, NS, max_cells, seed, amount_q, samples, scale_ids, (hipStream_t)stream));
    return 0;
}

// include/vtamiq_hip_weighted_sampler.h: the cell geometry (cs, sh, sw) of an h x w level, checked the same way by both entries
static const char* bad_cells(int32_t P, int32_t cs, int32_t sh, int32_t sw, int64_t hm, int64_t wm) {
    if (cs < 1 || cs < 3 * P / 4) return "cs < max(1, 3 P / 4)";
    if (sh != std::max<int64_t>(1, (hm + cs - 1) / cs) || sw != std::max<int64_t>(1, (wm + cs - 1) / cs)) return "sh, sw are not max(1, ceil((dim - P) / cs))";
    if ((int64_t)sh * sw > VTQ_WSAMPLER_MAX_CELLS) return "more than 8192 cells";
    return nullptr;
}

int vtq_k_diff_cells(const uint8_t* images, int64_t image_bytes, const int64_t* pairs, const int32_t* lev, const int64_t* pairs_host,
                     const int32_t* lev_host, int32_t NP, int32_t NL, int32_t P, uint64_t* tab, int64_t tab_words, void* stream) {
    if (!images || !pairs || !lev || !pairs_host || !lev_host || !tab) return fail("vtq_k_diff_cells: null argument");
    if ((uintptr_t)lev % 16) return fail("vtq_k_diff_cells: lev is not 16-byte aligned");
    if (NP < 1 || NP > 65535 || NL < 1) return fail("vtq_k_diff_cells: NP=%d (1 .. 65535), NL=%d (at least 1)", (int)NP, (int)NL);
    if (P < 8 || P > 64) return fail("vtq_k_diff_cells: patch size %d (8 .. 64)", (int)P);
    int64_t T = 0, max_pixels = 0;
    int32_t row = 0;
    for (int32_t p = 0; p < NP; ++p) {
        const int64_t* q = pairs_host + (int64_t)p * 8;
        const int64_t H = q[2], W = q[3];
        if (H < P || W < P || H > VTQ_WSAMPLER_MAX_PIXELS || W > VTQ_WSAMPLER_MAX_PIXELS || H * W > VTQ_WSAMPLER_MAX_PIXELS)
            return fail("vtq_k_diff_cells: pair %d is %lld x %lld (a patch of %d at least, %d pixels at most)", (int)p, (long long)H, (long long)W,
                        (int)P, VTQ_WSAMPLER_MAX_PIXELS);
        for (int k = 0; k < 2; ++k)
            if (q[k] < 0 || image_bytes < 0 || q[k] > image_bytes || 3 * H * W > image_bytes - q[k])
                return fail("vtq_k_diff_cells: pair %d, image %d (%lld x %lld at byte %lld) leaves the buffer of %lld bytes", (int)p, k, (long long)H,
                            (long long)W, (long long)q[k], (long long)image_bytes);
        if (q[4] != T) return fail("vtq_k_diff_cells: pair %d has its head at %lld, the table before it ends at %lld", (int)p, (long long)q[4], (long long)T);
        T += 4;
        if (q[5] != row) return fail("vtq_k_diff_cells: pair %d starts at row %lld of lev, the rows before it end at %d", (int)p, (long long)q[5], (int)row);
        int32_t last = -1, cnt = 0;
        for (; row < NL && lev_host[(int64_t)row * 8] == p; ++row, ++cnt) {
            const int32_t* t = lev_host + (int64_t)row * 8;
            const int32_t level = t[1], cs = t[2], sh = t[3], sw = t[4];
            if (level <= last || level > 3) return fail("vtq_k_diff_cells: row %d of lev is level %d (0 .. 3, increasing within a pair)", (int)row, (int)level);
            last = level;
            const int64_t h = H >> level, w = W >> level;
            if (h < P || w < P) return fail("vtq_k_diff_cells: row %d of lev: level %d of pair %d is %lld x %lld, below a patch", (int)row, (int)level, (int)p, (long long)h, (long long)w);
            if (const char* why = bad_cells(P, cs, sh, sw, h - P, w - P)) return fail("vtq_k_diff_cells: row %d of lev: %s", (int)row, why);
            if (t[5] != q[4] || t[6] != T) return fail("vtq_k_diff_cells: row %d of lev has head %d, tab_off %d (%lld, %lld expected)", (int)row, (int)t[5], (int)t[6], (long long)q[4], (long long)T);
            T += 2 + (int64_t)sh * sw;
            if (T > 0x7fffffff) return fail("vtq_k_diff_cells: a table above 2^31 - 1 words");
        }
        if (cnt < 1 || q[6] != cnt) return fail("vtq_k_diff_cells: pair %d has %d rows in lev and says %lld (at least 1)", (int)p, (int)cnt, (long long)q[6]);
        max_pixels = std::max(max_pixels, H * W);
    }
    if (row != NL) return fail("vtq_k_diff_cells: row %d of lev belongs to pair %d (pairs 0 .. %d in order)", (int)row, (int)lev_host[(int64_t)row * 8], (int)NP - 1);
    if (T != tab_words) return fail("vtq_k_diff_cells: the table has %lld words, tab_words=%lld", (long long)T, (long long)tab_words);
    HIP_TRY(launch_diff_cells(images, pairs, lev, NP, max_pixels, P, tab, tab_words, (hipStream_t)stream));
    return 0;
}

int vtq_k_sample_weighted(const int32_t* seg, const uint64_t* keys, const int32_t* seg_host, const uint64_t* keys_host, int32_t NS, int32_t P,
                          const uint64_t* tab, int64_t tab_words, double dw, double uw, uint64_t seed, int32_t amount_q, int32_t* samples,
                          int32_t* scale_ids, void* stream) {
    if (!seg || !keys || !seg_host || !keys_host || !samples) return fail("vtq_k_sample_weighted: null argument");
    if ((uintptr_t)seg % 16) return fail("vtq_k_sample_weighted: seg is not 16-byte aligned");
    if (NS < 1) return fail("vtq_k_sample_weighted: NS=%d (at least 1)", (int)NS);
    if (P < 8 || P > 64) return fail("vtq_k_sample_weighted: patch size %d (8 .. 64)", (int)P);
    if (amount_q < 0 || amount_q > 65535) return fail("vtq_k_sample_weighted: amount_q=%d (0 .. 65535)", (int)amount_q);
    if (!(dw >= 0.0) || !(uw >= 0.0) || !std::isfinite(dw) || !std::isfinite(uw) || dw + uw < 1e-6)
        return fail("vtq_k_sample_weighted: weights dw=%g, uw=%g (finite, not negative, a sum of 1e-6 at least)", dw, uw);
    int64_t total = 0;
    int max_cells = 0;
    for (int32_t j = 0; j < NS; ++j) {
        const int32_t* t = seg_host + (int64_t)j * 12;
        const int32_t first = t[0], n = t[1], cs = t[2], sh = t[3], sw = t[4], hm = t[5], wm = t[6], level = t[7], head = t[8], off = t[9];
        if (n < 1 || n > VTQ_WSAMPLER_MAX_SAMPLES) return fail("vtq_k_sample_weighted: segment %d asks for %d samples (1 .. %d)", (int)j, (int)n, VTQ_WSAMPLER_MAX_SAMPLES);
        if (hm < 0 || wm < 0 || hm >= VTQ_WSAMPLER_MAX_PIXELS || wm >= VTQ_WSAMPLER_MAX_PIXELS)
            return fail("vtq_k_sample_weighted: segment %d has h - P = %d, w - P = %d (0 .. %d)", (int)j, (int)hm, (int)wm, VTQ_WSAMPLER_MAX_PIXELS - 1);
        if (const char* why = bad_cells(P, cs, sh, sw, hm, wm)) return fail("vtq_k_sample_weighted: segment %d: %s", (int)j, why);
        if (level < 0 || level > 3) return fail("vtq_k_sample_weighted: segment %d is on level %d (0 .. 3)", (int)j, (int)level);
        if (level != 0 && !scale_ids) return fail("vtq_k_sample_weighted: scale_ids are required when a segment is on level %d", (int)level);
        if (first != total) return fail("vtq_k_sample_weighted: segment %d starts at row %d, the segments before it end at %lld", (int)j, (int)first, (long long)total);
        total += n;
        if (total > 0x7fffffff) return fail("vtq_k_sample_weighted: more than 2^31 - 1 samples");
        if (!(head == -1 && off == -1)) {
            if (head < 0 || off < 0 || (int64_t)head + 4 > tab_words || (int64_t)off + 2 + (int64_t)sh * sw > tab_words)
                return fail("vtq_k_sample_weighted: segment %d reads the table at %d and %d, beyond its %lld words", (int)j, (int)head, (int)off, (long long)tab_words);
            if (!tab && dw > 0.0) return fail("vtq_k_sample_weighted: segment %d has a table, diff_weight is %g and tab is NULL", (int)j, dw);
        }
        max_cells = std::max(max_cells, sh * sw);
    }
    HIP_TRY(launch_sample_weighted(seg, keys, NS, max_cells, P, tab, dw, uw, seed, amount_q, samples, scale_ids, (hipStream_t)stream));
    return 0;
}

}  // extern "C"
