// Transformer recogniser (TrOCR) handle: checkpoint ingest, graph, workspace and the vtd_trocr_* entry points of include/vtd.h.
// Textually included at the end of vtd_api.cpp (it shares that file's ModelBase / build_linear and its conv_select.h kernel selection).
// Reference: app/ml/models/text_recognizer.py:39-69 -> transformers 4.36 ViTModel + TrOCRForCausalLM + greedy generate
// (algorithm restated in oracle/trocr.py; kernels in trocr.hip).

struct TrocrCrop {
    int frame, x0, y0, w, h;
    int xtab, ytab;
    int ksx, ksy;
};
int vtd_launch_trocr_resample(const uint8_t* frames, int H, int W, const TrocrCrop* crops_dev, const int* pool, half_t* out, int ncrops, int S,
                              int P, int rows_per_block, int lds_rows, hipStream_t s);
int vtd_launch_trocr_pixels(const float* x, half_t* out, int n, int S, int P, hipStream_t s);
int vtd_launch_trocr_tokens(const float* patch, int ld_patch, const float* cls, const float* pos, float* stream, int n, int T, int C, hipStream_t s);
int vtd_launch_trocr_ln(float* x, const float* y, int ldy, const float* gamma, const float* beta, half_t* out16, float* out32, int rows, int C,
                        float eps, int mode, int64_t out16_prows, hipStream_t s);
int vtd_launch_trocr_attention(const half_t* qkv, half_t* out, int n, int T, int C, int heads, int64_t out_prows, hipStream_t s);
// csrc/dense_gemm.hip
int vtd_launch_dense_gemm_ex(const half_t* A, int lda, int64_t a_prows, const half_t* W, int w_rows, int w_panel, const float* bias, void* out, int ldc,
                             int64_t out_prows, int64_t M, int N, int K, int flags, hipStream_t stream);
bool vtd_dense_gemm_supported(int64_t M, int N, int K, int lda, int ldc, int flags);
int vtd_launch_dense_gemm(const half_t* A, int lda, const half_t* W, int w_rows, const float* bias, void* out, int ldc, int64_t M, int N, int K,
                          int flags, hipStream_t stream);
// csrc/trocr_decode.hip: the decoder chain on a compact list of live rows
int vtd_launch_dec_gemm(const half_t* A, int lda, const half_t* W, const float* bias, void* out, int ldc, int64_t slab_stride, int M,
                        const int* n_rows_dev, int N, int K, int ksplit, int flags, int wide, hipStream_t s);
int vtd_launch_dec_ln(float* x, half_t* x16, const float* slabs, int64_t slab_stride, int nsplit, const float* bias, const float* gamma,
                      const float* beta, const int* n_rows_dev, int M, int D, float eps, const float* embed, const float* pos, const int32_t* ids,
                      const int32_t* active, int ld_ids, int col, int position, int vocab, hipStream_t s);
int vtd_launch_dec_attn(int self, const half_t* q, int ldq, half_t* kc, half_t* vc, int64_t crop_stride, int L, int D, half_t* out,
                        const int32_t* active, const int* n_rows_dev, int M, int heads, hipStream_t s);
int vtd_launch_dec_argmax(const float* logits, int64_t ld, int V, int32_t* best_tok, const int* n_rows_dev, int M, hipStream_t s);
int vtd_launch_dec_advance(const int32_t* best_tok, int32_t* ids, int ld_ids, int col, int32_t* done, int32_t* active, int* n_rows_dev,
                           int* host_rows, const int32_t* forced, int ld_forced, int forced_len, int eos, int pad, int compact, hipStream_t s);
int vtd_launch_dec_init(int32_t* ids, int ld_ids, int32_t* done, int32_t* active, int* n_rows_dev, int n, int start, int pad, hipStream_t s);
// csrc/trocr_xattn.hip: cross-attention on the raw encoder states (composed query -> attention over E -> value projection)
bool vtd_dec_xattn_supported(int H, int T, int C);
int vtd_launch_dec_xq(const half_t* q, int ldq, const half_t* wkt, half_t* qp, const int* n_rows_dev, int M, int H, int C, hipStream_t s);
int vtd_launch_dec_xattn(const half_t* qp, const half_t* enc, half_t* cp, const int32_t* active, const int* n_rows_dev, int M, int H, int T, int C,
                         hipStream_t s);
int vtd_launch_dec_xv(const half_t* cp, const half_t* wv, const float* bv, half_t* out, const int* n_rows_dev, int M, int H, int C, int D,
                      hipStream_t s);

struct TrocrLN {
    float* g = nullptr;
    float* b = nullptr;
};

struct TrocrEncLayer {
    ConvOp qkv, o, fc1, fc2;
    TrocrLN before, after;
};

constexpr int kTrocrSlots = 2;     // encoder-output slots: the encoder pass of batch i+1 runs while batch i is decoded
constexpr int kDecSplitMax = 8;    // split-K slabs of the decoder's N = D projections
constexpr int kRowRing = 1024;     // pinned words for the live-row counts: word s = live rows after step s (max_length <= kRowRing)

struct TrocrDecLayer {
    // weights / biases only are taken from these ops ([N padded to 64][K] fp16, build_linear); the decoder chain runs on dec_gemm
    ConvOp sqkv, so, cq, co, fc1, fc2;
    ConvOp ck, cv;             // cross-attention keys / values of the encoder states: part of the encoder pass (implicit-GEMM path)
    TrocrLN ln_self, ln_cross, ln_final;
    half_t* kcache = nullptr;  // [max_crops][max_length][D]
    half_t* vcache = nullptr;
    half_t* ck_buf[kTrocrSlots] = {nullptr, nullptr};  // [max_crops * T][D] per slot
    half_t* cv_buf[kTrocrSlots] = {nullptr, nullptr};
    // cross-attention on the raw encoder states (vtd_trocr::xattn, trocr_xattn.hip): the key projection's weights per head, transposed
    // ([H][C][64]), the value projection's as they are ([D][C]) with its bias
    half_t* wkt = nullptr;
    half_t* wv16 = nullptr;
    float* bv = nullptr;
};

struct vtd_trocr : vtd::ModelBase {
    vtd_trocr_config cfg;
    int max_crops = 0, rows_pad = 0;
    bool xattn = true;          // decoder cross-attention on the raw encoder states instead of per-layer key / value projections (option "xattn";
                                // finalize falls back to the key / value form for an encoder the kernel does not cover, unless the option was 2)
    bool xattn_forced = false;
    bool dense_panel = true;    // K-panel-major inputs / weights of the encoder's dense GEMMs (VTD_DENSE_PANEL=0 at finalize: row-major everywhere)
    half_t* enc16[kTrocrSlots] = {nullptr, nullptr};   // xattn: final encoder states [max_crops][T][C] fp16 per slot (0.89 MB per crop instead of 28 MB)
    half_t *qp16 = nullptr, *cp16 = nullptr;           // xattn: composed queries / attended encoder states [rows][H * C]
    int n_slots = 1;            // encoder-output slots in use (vtd_trocr_set_option "slots": 2 lets an encoder pass run while another batch waits for / runs its decode)
    bool finalized = false;
    int T = 0, NP = 0, PK = 0;  // encoder tokens, patches, patch vector length (3 * P * P)
    int vld = 0;                // row stride of the logits buffer (vocab rounded up to 4)
    float *cls = nullptr, *pos_enc = nullptr;
    ConvOp patch;
    std::vector<TrocrEncLayer> enc;
    TrocrLN enc_final, ln_emb;
    float *embed = nullptr, *pos_dec = nullptr;
    std::vector<TrocrDecLayer> dec;
    ConvOp lm_head;
    // encoder workspace (one: encoder passes serialise on enc_free)
    half_t *patches = nullptr, *ln16 = nullptr, *qkv = nullptr, *att16 = nullptr, *ffn16 = nullptr, *kv_home = nullptr;
    float *patch_out = nullptr, *stream = nullptr, *y32 = nullptr, *enc_out32 = nullptr;
    // decoder workspace (one: decodes serialise on dec_free), rows = position in the live list
    float *dstream = nullptr, *slabs = nullptr, *logits = nullptr;
    half_t *d16 = nullptr, *qkv16 = nullptr, *q16 = nullptr, *datt16 = nullptr, *dffn16 = nullptr;
    int32_t *done = nullptr, *active = nullptr, *best_tok = nullptr;
    int* n_rows = nullptr;       // device: live rows
    int* host_rows = nullptr;    // pinned host: word s = live rows after step s of the current generate call (written by its dec_advance)
    hipEvent_t enc_done[kTrocrSlots] = {nullptr, nullptr}, dec_done[kTrocrSlots] = {nullptr, nullptr};
    hipEvent_t enc_free = nullptr, dec_free = nullptr, step_ev[3] = {nullptr, nullptr, nullptr};
    bool enc_used = false, dec_used = false, slot_enc[kTrocrSlots] = {false, false}, slot_dec[kTrocrSlots] = {false, false};
    int last_steps = 0;          // steps the last generate enqueued (diagnostics / tests)
    // profiling of the cross-attention launches (bench.py: roofline of the TrOCR line)
    int prof_mode = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_ev;
    std::vector<std::pair<int, int>> prof_rows;   // (step, crops of the call): rows the launch read = live rows after step - 1
    std::vector<int> prof_exact;
    size_t prof_used = 0;
    // ... and of the encoder pass's dense-GEMM launches (prof_mode bit 1): events on the encoder's stream + the FLOPs each launch executes
    std::vector<std::pair<hipEvent_t, hipEvent_t>> gprof_ev;
    std::vector<double> gprof_flops;
    size_t gprof_used = 0;
    TrocrCrop* crops_dev = nullptr;
    int* pool = nullptr;
    size_t pool_cap = 0, pool_used = 0;
    std::map<int, std::pair<int, int>> axis;  // input extent -> (pool offset, ksize)
    TrocrCrop* crops_pin[kTrocrSlots] = {nullptr, nullptr};   // pinned staging of the crop table, one per slot
    std::map<int, std::map<std::string, int>> tuned;  // bucket -> launch-slot name -> config
    int64_t macs = 0;
    ~vtd_trocr() {
        for (int i = 0; i < kTrocrSlots; ++i) {
            if (enc_done[i]) (void)hipEventDestroy(enc_done[i]);
            if (dec_done[i]) (void)hipEventDestroy(dec_done[i]);
        }
        if (enc_free) (void)hipEventDestroy(enc_free);
        if (dec_free) (void)hipEventDestroy(dec_free);
        for (auto& e : step_ev)
            if (e) (void)hipEventDestroy(e);
        for (auto& pr : prof_ev) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
        for (auto& pr : gprof_ev) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
        if (host_rows) (void)hipHostFree(host_rows);
        for (auto& c : crops_pin)
            if (c) (void)hipHostFree(c);
    }
};

namespace vtd {

static std::vector<float> tr_bias_or_zero(const ModelBase* m, const std::string& key, int n, bool* present = nullptr) {
    auto it = m->sd.find(key);
    if (present) *present = it != m->sd.end();
    if (it == m->sd.end()) return std::vector<float>(n, 0.f);
    return it->second;
}

static int tr_upload_vec(vtd_trocr* t, const std::string& key, size_t numel, float** dev) {
    auto v = t->get(key, numel);
    if (!v) return ERR_MISSING_KEY;
    return upload(t->arena, v->data(), numel * sizeof(float), (void**)dev);
}

static int tr_ln(vtd_trocr* t, const std::string& prefix, int c, TrocrLN& ln) {
    int rc;
    if ((rc = tr_upload_vec(t, prefix + ".weight", c, &ln.g))) return rc;
    return tr_upload_vec(t, prefix + ".bias", c, &ln.b);
}

// Linear layer `prefix` ([N][K] weight, optional bias) over the rows of `in`; `scale` folds a power-of-two factor into weight and bias
// `home` / `home_ld`: a destination that is safe for max_crops rows -- what the kernel-selection contest writes to (launches pass
// their own destination, which may be sized for the actual crop count only)
// The weights of a dense layer once more, K-panel-major ([K / 32][cout_pad][32] fp16, zero rows up to cout_pad): what dense_gemm.hip streams
// when the encoder pass runs on panels (fp32 -> fp16 exactly as build_linear rounds them: the same values).
static int tr_panel_weights(vtd_trocr* t, ConvOp& op, const std::vector<float>& W, int N, int K) {
    if (!t->dense_panel || (K & 31)) return 0;
    const int cp = op.cout_pad;
    std::vector<half_t> wp((size_t)cp * K, (half_t)0.f);
    for (int n = 0; n < N; ++n)
        for (int k = 0; k < K; ++k) wp[((size_t)(k >> 5) * cp + n) * 32 + (k & 31)] = (half_t)W[(size_t)n * K + k];
    return upload(t->arena, wp.data(), wp.size() * sizeof(half_t), (void**)&op.w_panel);
}

static int tr_linear(vtd_trocr* t, ConvOp& op, const TensorDesc& in, const std::string& prefix, int N, int K, int flags, void* home, int home_ld,
                     float scale = 1.f, bool bias_required = true, bool panel_copy = false) {
    auto w = t->get(prefix + ".weight", (size_t)N * K);
    if (!w) return ERR_MISSING_KEY;
    bool have = false;
    std::vector<float> b = tr_bias_or_zero(t, prefix + ".bias", N, &have);
    if (!have && bias_required) return ERR_MISSING_KEY;
    if ((int)b.size() != N) return ERR_SHAPE;
    std::vector<float> ws(*w);
    if (scale != 1.f) {
        for (float& v : ws) v *= scale;
        for (float& v : b) v *= scale;
    }
    const int rc = build_linear(t, op, in, ws, b, N, K, home, home_ld, flags);
    if (rc || !panel_copy) return rc;
    return tr_panel_weights(t, op, ws, N, K);
}

template <typename Tp>
static int tr_alloc(vtd_trocr* t, Tp** p, size_t elems) {
    void* v = nullptr;
    int rc = t->arena.alloc(&v, elems * sizeof(Tp), true);
    *p = (Tp*)v;
    return rc;
}

static int build_trocr_graph(vtd_trocr* t) {
    const vtd_trocr_config& c = t->cfg;
    if (const char* e = std::getenv("VTD_DENSE_PANEL"); e && e[0] == '0') t->dense_panel = false;
    const int S = c.image_size, P = c.patch_size, C = c.enc_hidden, F = c.enc_ffn, D = c.dec_hidden, DF = c.dec_ffn, V = c.vocab_size;
    const int mc = t->max_crops, L = c.max_length;
    if (S % P || (C & 63) || (F & 63) || (D & 63) || (DF & 63) || C != c.enc_heads * 64 || D != c.dec_heads * 64 || ((3 * P * P) & 63) ||
        C > 2048 || D > 2048 || L < 2 || L > c.max_positions || L > kRowRing || mc > 4096)
        return ERR_GEOMETRY;
    t->NP = (S / P) * (S / P);
    t->T = t->NP + 1;
    t->PK = 3 * P * P;
    t->vld = (V + 3) & ~3;
    const int T = t->T, NP = t->NP;
    int rc;
    // ---- workspace (decoder rows are rounded up to the 64-row tile of dec_gemm: rows past the live count are read, never written)
    t->rows_pad = (mc + 63) / 64 * 64;
    const size_t rp = (size_t)t->rows_pad;
    if ((rc = tr_alloc(t, &t->patches, (size_t)mc * NP * t->PK)) || (rc = tr_alloc(t, &t->patch_out, (size_t)mc * NP * C)) ||
        (rc = tr_alloc(t, &t->stream, (size_t)mc * T * C)) || (rc = tr_alloc(t, &t->ln16, (size_t)mc * T * C)) ||
        (rc = tr_alloc(t, &t->qkv, (size_t)mc * T * 3 * C)) || (rc = tr_alloc(t, &t->att16, (size_t)mc * T * C)) ||
        (rc = tr_alloc(t, &t->y32, (size_t)mc * T * C)) || (rc = tr_alloc(t, &t->ffn16, (size_t)mc * T * F)) ||
        (rc = tr_alloc(t, &t->enc_out32, (size_t)mc * T * C)) || (rc = tr_alloc(t, &t->kv_home, (size_t)mc * T * D)) ||
        (rc = tr_alloc(t, &t->dstream, rp * D)) || (rc = tr_alloc(t, &t->slabs, (size_t)kDecSplitMax * rp * D)) ||
        (rc = tr_alloc(t, &t->d16, rp * D)) || (rc = tr_alloc(t, &t->qkv16, rp * 3 * D)) || (rc = tr_alloc(t, &t->q16, rp * D)) ||
        (rc = tr_alloc(t, &t->datt16, rp * D)) || (rc = tr_alloc(t, &t->dffn16, rp * DF)) ||
        (rc = tr_alloc(t, &t->logits, rp * t->vld)) || (rc = tr_alloc(t, &t->done, (size_t)mc)) || (rc = tr_alloc(t, &t->active, rp)) ||
        (rc = tr_alloc(t, &t->best_tok, rp)) || (rc = tr_alloc(t, &t->n_rows, 4)) || (rc = tr_alloc(t, &t->crops_dev, (size_t)mc)))
        return rc;
    if (t->xattn && !vtd_dec_xattn_supported(c.dec_heads, T, C)) {
        if (t->xattn_forced) return ERR_GEOMETRY;
        t->xattn = false;
    }
    if (t->xattn) {
        for (int sl = 0; sl < t->n_slots; ++sl)
            if ((rc = tr_alloc(t, &t->enc16[sl], (size_t)mc * T * C))) return rc;
        if ((rc = tr_alloc(t, &t->qp16, rp * c.dec_heads * C)) || (rc = tr_alloc(t, &t->cp16, rp * c.dec_heads * C))) return rc;
    }
    VTD_HIP_CHECK(hipHostMalloc((void**)&t->host_rows, kRowRing * sizeof(int), hipHostMallocDefault));   // one word per step of a generate call
    std::memset(t->host_rows, 0, kRowRing * sizeof(int));
    for (auto& cp : t->crops_pin) VTD_HIP_CHECK(hipHostMalloc((void**)&cp, (size_t)mc * sizeof(TrocrCrop), hipHostMallocDefault));
    for (int i = 0; i < kTrocrSlots; ++i) {
        VTD_HIP_CHECK(hipEventCreateWithFlags(&t->enc_done[i], hipEventDisableTiming));
        VTD_HIP_CHECK(hipEventCreateWithFlags(&t->dec_done[i], hipEventDisableTiming));
    }
    VTD_HIP_CHECK(hipEventCreateWithFlags(&t->enc_free, hipEventDisableTiming));
    VTD_HIP_CHECK(hipEventCreateWithFlags(&t->dec_free, hipEventDisableTiming));
    for (auto& e : t->step_ev) VTD_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    t->pool_cap = (size_t)4 << 20;  // 4M ints of resample coefficients (grown on demand)
    if ((rc = tr_alloc(t, &t->pool, t->pool_cap))) return rc;
    // ---- encoder
    const std::string e = "encoder.embeddings.";
    if ((rc = tr_upload_vec(t, e + "cls_token", C, &t->cls)) || (rc = tr_upload_vec(t, e + "position_embeddings", (size_t)T * C, &t->pos_enc))) return rc;
    TensorDesc d_patch = make_desc(mc, 1, NP, t->PK, 0, 0);
    d_patch.ptr = t->patches;
    if ((rc = tr_linear(t, t->patch, d_patch, e + "patch_embeddings.projection", C, t->PK, EPI_OUT_F32, t->patch_out, C))) return rc;
    t->macs += (int64_t)NP * C * t->PK;
    TensorDesc d_tok = make_desc(mc, 1, T, C, 0, 0), d_ffn = make_desc(mc, 1, T, F, 0, 0);
    d_tok.ptr = t->ln16;
    d_ffn.ptr = t->ffn16;
    TensorDesc d_att = d_tok;
    d_att.ptr = t->att16;
    t->enc.resize(c.enc_layers);
    for (int i = 0; i < c.enc_layers; ++i) {
        const std::string p = "encoder.encoder.layer." + std::to_string(i) + ".";
        TrocrEncLayer& l = t->enc[i];
        {   // q | k | v as one [3C][C] GEMM
            std::vector<float> W((size_t)3 * C * C), B(3 * C, 0.f);
            const char* names[3] = {"query", "key", "value"};
            for (int j = 0; j < 3; ++j) {
                auto w = t->get(p + "attention.attention." + names[j] + ".weight", (size_t)C * C);
                if (!w) return ERR_MISSING_KEY;
                std::copy(w->begin(), w->end(), W.begin() + (size_t)j * C * C);
                auto b = t->sd.find(p + "attention.attention." + names[j] + ".bias");
                if (b != t->sd.end()) {
                    if ((int)b->second.size() != C) return ERR_SHAPE;
                    std::copy(b->second.begin(), b->second.end(), B.begin() + j * C);
                } else if (c.enc_qkv_bias) {
                    return ERR_MISSING_KEY;
                }
            }
            if ((rc = build_linear(t, l.qkv, d_tok, W, B, 3 * C, C, t->qkv, 3 * C, EPI_OUT_F16)) || (rc = tr_panel_weights(t, l.qkv, W, 3 * C, C))) return rc;
        }
        if ((rc = tr_linear(t, l.o, d_att, p + "attention.output.dense", C, C, EPI_OUT_F32, t->y32, C, 1.f, true, true)) ||
            (rc = tr_linear(t, l.fc1, d_tok, p + "intermediate.dense", F, C, EPI_OUT_F16 | EPI_GELU, t->ffn16, F, 1.f, true, true)) ||
            (rc = tr_linear(t, l.fc2, d_ffn, p + "output.dense", C, F, EPI_OUT_F32, t->y32, C, 1.f, true, true)) || (rc = tr_ln(t, p + "layernorm_before", C, l.before)) ||
            (rc = tr_ln(t, p + "layernorm_after", C, l.after)))
            return rc;
        t->macs += (int64_t)T * ((int64_t)3 * C * C + (int64_t)C * C + (int64_t)2 * C * F) + (int64_t)2 * T * T * C;
    }
    if ((rc = tr_ln(t, "encoder.layernorm", C, t->enc_final))) return rc;
    // ---- decoder
    const std::string q = "decoder.model.decoder.";
    if ((rc = tr_upload_vec(t, q + "embed_tokens.weight", (size_t)V * D, &t->embed)) ||
        (rc = tr_upload_vec(t, q + "embed_positions.weight", (size_t)(c.max_positions + 2) * D, &t->pos_dec)) ||
        (rc = tr_ln(t, q + "layernorm_embedding", D, t->ln_emb)))
        return rc;
    TensorDesc d_enc = make_desc(mc, 1, T, C, 0, 0);   // final encoder states (fp16) feed the cross k / v projections
    d_enc.ptr = t->ln16;
    TensorDesc d_row = make_desc(mc, 1, 1, D, 0, 0), d_rowatt = d_row, d_rowffn = make_desc(mc, 1, 1, DF, 0, 0);
    d_row.ptr = t->d16;
    d_rowatt.ptr = t->datt16;
    d_rowffn.ptr = t->dffn16;
    const float scaling = 0.125f;  // head_dim ** -0.5, applied to q after its bias (TrOCRAttention.forward)
    t->dec.resize(c.dec_layers);
    for (int i = 0; i < c.dec_layers; ++i) {
        const std::string p = q + "layers." + std::to_string(i) + ".";
        TrocrDecLayer& l = t->dec[i];
        if ((rc = tr_alloc(t, &l.kcache, (size_t)mc * L * D)) || (rc = tr_alloc(t, &l.vcache, (size_t)mc * L * D))) return rc;
        for (int sl = 0; sl < t->n_slots && !t->xattn; ++sl)   // 28 MB per crop and slot over the 12 layers: the second slot only when it was asked for
            if ((rc = tr_alloc(t, &l.ck_buf[sl], (size_t)mc * T * D)) || (rc = tr_alloc(t, &l.cv_buf[sl], (size_t)mc * T * D))) return rc;
        if (t->xattn) {
            // cross-attention on the raw encoder states: Wk per head transposed ([H][C][64]: the composed query's MFMA reads 64-deep rows),
            // Wv as it is, bv; bk is not needed (q . bk is the same for every token of a row: the softmax drops it)
            auto wk = t->get(p + "encoder_attn.k_proj.weight", (size_t)D * C), wv = t->get(p + "encoder_attn.v_proj.weight", (size_t)D * C);
            if (!wk || !wv || !t->get(p + "encoder_attn.k_proj.bias", D)) return ERR_MISSING_KEY;
            const std::vector<float> bvv = tr_bias_or_zero(t, p + "encoder_attn.v_proj.bias", D);
            if ((int)bvv.size() != D) return ERR_SHAPE;
            const int H = c.dec_heads;
            std::vector<half_t> wkt((size_t)H * C * 64), wv16((size_t)D * C);
            for (int h = 0; h < H; ++h)
                for (int e = 0; e < C; ++e)
                    for (int dd = 0; dd < 64; ++dd) wkt[((size_t)h * C + e) * 64 + dd] = (half_t)(*wk)[(size_t)(h * 64 + dd) * C + e];
            for (size_t i = 0; i < (size_t)D * C; ++i) wv16[i] = (half_t)(*wv)[i];
            if ((rc = upload(t->arena, wkt.data(), wkt.size() * sizeof(half_t), (void**)&l.wkt)) ||
                (rc = upload(t->arena, wv16.data(), wv16.size() * sizeof(half_t), (void**)&l.wv16)) ||
                (rc = upload(t->arena, bvv.data(), bvv.size() * sizeof(float), (void**)&l.bv)))
                return rc;
        }
        // The decoder's dense layers: weights packed by build_linear ([N padded to 64][K] fp16 + padded fp32 bias); they run on dec_gemm
        // (trocr_decode.hip), the `home` destinations below only size-check the geometry.  kv_home is a scratch destination for the
        // kernel-selection contest of the ck / cv launch slots (a contest must never write into a slot another stream is decoding from).
        if ((rc = tr_linear(t, l.so, d_rowatt, p + "self_attn.out_proj", D, D, EPI_OUT_F32, t->slabs, D)) ||
            (rc = tr_linear(t, l.cq, d_row, p + "encoder_attn.q_proj", D, D, EPI_OUT_F16, t->q16, D, scaling)) ||
            (rc = tr_linear(t, l.ck, d_enc, p + "encoder_attn.k_proj", D, C, EPI_OUT_F16, t->kv_home, D, 1.f, true, !t->xattn)) ||
            (rc = tr_linear(t, l.cv, d_enc, p + "encoder_attn.v_proj", D, C, EPI_OUT_F16, t->kv_home, D, 1.f, true, !t->xattn)) ||
            (rc = tr_linear(t, l.co, d_rowatt, p + "encoder_attn.out_proj", D, D, EPI_OUT_F32, t->slabs, D)) ||
            (rc = tr_linear(t, l.fc1, d_row, p + "fc1", DF, D, EPI_OUT_F16 | EPI_GELU, t->dffn16, DF)) ||
            (rc = tr_linear(t, l.fc2, d_rowffn, p + "fc2", D, DF, EPI_OUT_F32, t->slabs, D)) || (rc = tr_ln(t, p + "self_attn_layer_norm", D, l.ln_self)) ||
            (rc = tr_ln(t, p + "encoder_attn_layer_norm", D, l.ln_cross)) || (rc = tr_ln(t, p + "final_layer_norm", D, l.ln_final)))
            return rc;
        {   // self-attention q | k | v as ONE [3D][D] projection (the 0.125 on q is a power of two: exact in fp16)
            std::vector<float> W((size_t)3 * D * D), B(3 * D, 0.f);
            const char* names[3] = {"q_proj", "k_proj", "v_proj"};
            for (int j = 0; j < 3; ++j) {
                auto w = t->get(p + "self_attn." + names[j] + ".weight", (size_t)D * D);
                auto b = t->sd.find(p + "self_attn." + std::string(names[j]) + ".bias");
                if (!w || b == t->sd.end()) return ERR_MISSING_KEY;
                if ((int)b->second.size() != D) return ERR_SHAPE;
                const float sc = j == 0 ? scaling : 1.f;
                for (size_t e = 0; e < (size_t)D * D; ++e) W[(size_t)j * D * D + e] = (*w)[e] * sc;
                for (int e = 0; e < D; ++e) B[j * D + e] = b->second[e] * sc;
            }
            if ((rc = build_linear(t, l.sqkv, d_row, W, B, 3 * D, D, t->qkv16, 3 * D, EPI_OUT_F16))) return rc;
        }
        t->macs += (int64_t)2 * T * D * C;  // cross k / v once per crop; the per-step work is added by generate()'s caller view below
    }
    {   // output projection: untied when the checkpoint carries it, else the embedding matrix
        const std::string key = t->sd.count("decoder.output_projection.weight") ? "decoder.output_projection" : q + "embed_tokens";
        if ((rc = tr_linear(t, t->lm_head, d_row, key, V, D, EPI_OUT_F32, t->logits, t->vld, 1.f, false))) return rc;
    }
    // per generated token: 12 x (4 D^2 self + 2 D^2 cross q/out + 2 D DF) + V D; reported for max_length - 1 steps
    t->macs += (int64_t)(L - 1) * ((int64_t)c.dec_layers * ((int64_t)6 * D * D + (int64_t)2 * D * DF) + (int64_t)V * D);
    return 0;
}

// configuration of launch slot `name` at batch bucket `bucket` (table first, timing contest otherwise)
static int tr_cfg(vtd_trocr* t, const char* name, int layer, const ConvOp& op /* with its home destination */, int bucket, hipStream_t s) {
    std::string key = std::string(name) + "." + std::to_string(layer);
    auto& slot = t->tuned[bucket];
    auto it = slot.find(key);
    if (it != slot.end()) return it->second;
    int cfg = -1;
    if (choose_config(t, op, bucket, s, &cfg)) cfg = -1;
    slot[key] = cfg;
    return cfg;
}

// The encoder pass's dense layers at whole-batch token counts go to the 256 x 256 dense GEMM (dense_gemm.hip) when there are enough
// tiles to fill the chip (VTD_DENSE_GEMM=1: wherever the shape allows -- tests; =0: never); everything else stays on the implicit GEMM.
static bool tr_dense_wanted(const ConvOp& op, int64_t M, int ldc) {
    const int flags = op.flags & (EPI_OUT_F16 | EPI_OUT_F32 | EPI_GELU);
    if (op.flags != flags || op.in.c != op.K || op.in.ring != 0) return false;
    const char* e = std::getenv("VTD_DENSE_GEMM");
    if (e && e[0] == '0') return false;
    if (e && e[0] == '1') return M >= 256 && op.cout >= 256 && !(op.cout & 7) && !(op.K & 31) && op.K >= 128 && !(ldc & 7);
    return vtd_dense_gemm_supported(M, op.cout, op.K, op.K, ldc, flags);
}

// a_prows / out_prows: the A operand / the fp16 output are K-panel-major with that many rows (0: row-major) -- dense GEMM only
static int tr_launch(vtd_trocr* t, const char* name, int layer, const ConvOp& op, int n, int bucket, void* out, int ldc, hipStream_t s,
                     int64_t a_prows = 0, int64_t out_prows = 0) {
    const int64_t M = (int64_t)n * op.ho * op.wo;
    if (tr_dense_wanted(op, M, ldc)) {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (t->prof_mode & 2) {   // measurement only (bench.py: the Transformer lines' roofline is this kernel's)
            if (t->gprof_used == t->gprof_ev.size()) {
                hipEvent_t a = nullptr, b = nullptr;
                VTD_HIP_CHECK(hipEventCreate(&a));
                VTD_HIP_CHECK(hipEventCreate(&b));
                t->gprof_ev.push_back({a, b});
                t->gprof_flops.push_back(0.0);
            }
            e0 = t->gprof_ev[t->gprof_used].first; e1 = t->gprof_ev[t->gprof_used].second;
            t->gprof_flops[t->gprof_used] = 2.0 * (double)M * op.cout * op.K;
            ++t->gprof_used;
            VTD_HIP_CHECK(hipEventRecord(e0, s));
        }
        const bool wp = op.w_panel != nullptr && t->dense_panel;
        const int rc = vtd_launch_dense_gemm_ex(op.in.ptr, op.K, a_prows, wp ? op.w_panel : op.w, op.cout_pad, wp ? 1 : 0, op.bias, out, ldc, out_prows, M,
                                                op.cout, op.K, op.flags & (EPI_OUT_F16 | EPI_OUT_F32 | EPI_GELU), s);
        if (e1) VTD_HIP_CHECK(hipEventRecord(e1, s));
        return rc;
    }
    if (a_prows || out_prows) return ERR_GEOMETRY;   // (the caller asks for panels only when every consumer is a dense GEMM)
    const int cfg = tr_cfg(t, name, layer, op, bucket, s);
    ConvOp o = op;
    o.out_f32 = out;
    o.ldc = ldc;
    return launch_conv_op(o, n, s, cfg);
}

// Cross-stream ordering lives in the handle, not in the caller: an encoder pass waits for the previous encoder pass (one encoder
// workspace) and for the decode that last read its slot; a decode waits for its slot's encoder pass and for the previous decode (one
// decoder workspace).  So `encode(slot 1)` on one stream overlaps `generate(slot 0)` on another and nothing else needs to be said.
static int trocr_encoder_prologue(vtd_trocr* t, int slot, hipStream_t s) {
    if (t->enc_used) VTD_HIP_CHECK(hipStreamWaitEvent(s, t->enc_free, 0));
    if (t->slot_dec[slot]) VTD_HIP_CHECK(hipStreamWaitEvent(s, t->dec_done[slot], 0));
    return 0;
}

static int trocr_run_encoder(vtd_trocr* t, int slot, int n, hipStream_t s) {
    const vtd_trocr_config& c = t->cfg;
    const int C = c.enc_hidden, F = c.enc_ffn, D = c.dec_hidden, T = t->T;
    const int bucket = batch_bucket(n, t->max_crops);
    int rc;
    if ((rc = tr_launch(t, "patch", 0, t->patch, n, bucket, t->patch_out, C, s))) return rc;
    if ((rc = vtd_launch_trocr_tokens(t->patch_out, C, t->cls, t->pos_enc, t->stream, n, T, C, s))) return rc;
    const int rows = n * T;
    // K-panel-major GEMM inputs (dense_gemm.hip: an LDS-DMA piece is then 1 KB of contiguous memory instead of sixteen half cache lines): the
    // three fp16 buffers every dense layer reads -- LayerNorm output, attention output, GELU output -- are written [C / 32][rows][32] by their
    // producers when every consumer of the pass is a dense GEMM (whole-batch token counts; the reduced architectures and tiny passes stay
    // row-major on the implicit GEMM).  Same values, same products, same order: bit-identical results either way (VTD_DENSE_PANEL=0: off).
    bool panel = t->dense_panel && c.enc_layers > 0;
    if (panel) {
        const TrocrEncLayer& l0 = t->enc[0];
        panel = tr_dense_wanted(l0.qkv, rows, 3 * C) && tr_dense_wanted(l0.o, rows, C) && tr_dense_wanted(l0.fc1, rows, F) && tr_dense_wanted(l0.fc2, rows, C) &&
                l0.qkv.w_panel && l0.o.w_panel && l0.fc1.w_panel && l0.fc2.w_panel && !(C & 31) && !(F & 31);
        if (panel && !t->xattn && c.dec_layers > 0)
            panel = tr_dense_wanted(t->dec[0].ck, rows, D) && tr_dense_wanted(t->dec[0].cv, rows, D);
    }
    const int64_t pr = panel ? rows : 0;
    if ((rc = vtd_launch_trocr_ln(t->stream, nullptr, 0, t->enc[0].before.g, t->enc[0].before.b, t->ln16, nullptr, rows, C, c.enc_ln_eps, 0, pr, s)))
        return rc;
    for (int i = 0; i < c.enc_layers; ++i) {
        TrocrEncLayer& l = t->enc[i];
        if ((rc = tr_launch(t, "enc.qkv", i, l.qkv, n, bucket, t->qkv, 3 * C, s, pr))) return rc;
        if ((rc = vtd_launch_trocr_attention(t->qkv, t->att16, n, T, C, c.enc_heads, pr, s))) return rc;
        if ((rc = tr_launch(t, "enc.o", i, l.o, n, bucket, t->y32, C, s, pr))) return rc;
        if ((rc = vtd_launch_trocr_ln(t->stream, t->y32, C, l.after.g, l.after.b, t->ln16, nullptr, rows, C, c.enc_ln_eps, 1, pr, s))) return rc;
        if ((rc = tr_launch(t, "enc.fc1", i, l.fc1, n, bucket, t->ffn16, F, s, pr, pr))) return rc;
        if ((rc = tr_launch(t, "enc.fc2", i, l.fc2, n, bucket, t->y32, C, s, pr))) return rc;
        const bool last = i + 1 == c.enc_layers;
        const TrocrLN& nx = last ? t->enc_final : t->enc[i + 1].before;
        // (xattn: the decoder attends over the final encoder states themselves: they go straight into the slot, row-major)
        const bool to_slot = last && t->xattn;
        if ((rc = vtd_launch_trocr_ln(t->stream, t->y32, C, nx.g, nx.b, to_slot ? t->enc16[slot] : t->ln16, last ? t->enc_out32 : nullptr, rows, C,
                                      c.enc_ln_eps, 1, to_slot ? 0 : pr, s)))
            return rc;
    }
    // cross-attention keys / values of every decoder layer, once per crop (TrOCRAttention caches them after the first step)
    for (int i = 0; i < c.dec_layers && !t->xattn; ++i) {
        TrocrDecLayer& l = t->dec[i];
        if ((rc = tr_launch(t, "dec.ck", i, l.ck, n, bucket, l.ck_buf[slot], D, s, pr))) return rc;
        if ((rc = tr_launch(t, "dec.cv", i, l.cv, n, bucket, l.cv_buf[slot], D, s, pr))) return rc;
    }
    VTD_HIP_CHECK(hipEventRecord(t->enc_done[slot], s));
    VTD_HIP_CHECK(hipEventRecord(t->enc_free, s));
    t->slot_enc[slot] = true;
    t->enc_used = true;
    return 0;
}

static int trocr_axis(vtd_trocr* t, int in_size, int* off, int* ks) {
    auto it = t->axis.find(in_size);
    if (it != t->axis.end()) {
        *off = it->second.first;
        *ks = it->second.second;
        return 0;
    }
    ResampleAxis a = pillow_axis(in_size, t->cfg.image_size);
    const size_t need = a.bounds.size() + a.kk.size();
    if (t->pool_used + need > t->pool_cap) return ERR_CAPACITY;
    std::vector<int> packed(a.bounds);
    packed.insert(packed.end(), a.kk.begin(), a.kk.end());
    hipError_t e = hipMemcpy(t->pool + t->pool_used, packed.data(), need * sizeof(int), hipMemcpyHostToDevice);
    if (e != hipSuccess) return -(int)e;
    *off = (int)t->pool_used;
    *ks = a.ksize;
    t->axis[in_size] = {*off, *ks};
    t->pool_used += need;
    return 0;
}

}  // namespace vtd

extern "C" {

int vtd_trocr_create(const vtd_trocr_config* cfg, int max_crops, vtd_trocr** out) {
    if (!cfg || !out || max_crops <= 0 || cfg->image_size <= 0 || cfg->patch_size <= 0 || cfg->vocab_size <= 0 || cfg->enc_layers <= 0 ||
        cfg->dec_layers <= 0)
        return ERR_ARG;
    auto* t = new vtd_trocr();
    t->cfg = *cfg;
    t->max_crops = max_crops;
    *out = t;
    return 0;
}

void vtd_trocr_destroy(vtd_trocr* t) { delete t; }

int vtd_trocr_set_option(vtd_trocr* t, const char* name, int value) {
    if (!t || !name || t->finalized) return ERR_ARG;
    if (std::string(name) == "xattn") {
        if (value < 0 || value > 2) return ERR_ARG;
        t->xattn = value != 0;
        t->xattn_forced = value == 2;
        return 0;
    }
    if (std::string(name) == "slots") {
        if (value < 1 || value > kTrocrSlots) return ERR_ARG;
        t->n_slots = value;
        return 0;
    }
    return ERR_UNKNOWN_KEY;
}

int vtd_trocr_get_option(const vtd_trocr* t, const char* name, int* value) {
    if (!t || !name || !value) return ERR_ARG;
    if (std::string(name) == "xattn") { *value = t->xattn ? 1 : 0; return 0; }   // after finalize: the form that runs
    if (std::string(name) == "slots") { *value = t->n_slots; return 0; }
    return ERR_UNKNOWN_KEY;
}

int vtd_trocr_set_tensor(vtd_trocr* t, const char* key, const float* host_data, int64_t numel) {
    if (!t || !key || !host_data || numel < 0 || t->finalized) return ERR_ARG;
    const std::string k = key;
    if (k.rfind("encoder.", 0) != 0 && k.rfind("decoder.", 0) != 0) return ERR_UNKNOWN_KEY;
    if (k.rfind("encoder.pooler.", 0) == 0) return 0;  // never read by generate()
    t->sd[k].assign(host_data, host_data + numel);
    return 0;
}

int vtd_trocr_finalize(vtd_trocr* t, vtd_stream stream) {
    if (!t || t->finalized) return ERR_ARG;
    int rc = build_trocr_graph(t);
    if (rc) return rc;
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return -(int)e;
    t->sd.clear();
    t->finalized = true;
    return 0;
}

// The processor alone: crops of one resident frame batch -> patch-major pixel values, rows [row_offset, row_offset + ncrops) of the
// slot's next encoder pass.  Crops of SEVERAL frame batches (of different frame sizes, too) can be staged one call after the other and
// then encoded and decoded together (vtd_trocr_encode_staged_slot): the decode's cost per step is mostly fixed, so a recogniser batch
// that spans two detector batches costs little more than one.
int vtd_trocr_stage_crops_slot(vtd_trocr* t, int slot, const uint8_t* frames_dev, int n_frames, int height, int width, const int32_t* boxes_host,
                               int ncrops, int row_offset, vtd_stream stream) {
    if (!t || !frames_dev || !boxes_host || n_frames <= 0 || height <= 0 || width <= 0 || slot < 0 || slot >= t->n_slots || row_offset < 0)
        return ERR_ARG;
    if (!t->finalized) return ERR_NOT_FINALIZED;
    if (ncrops <= 0 || row_offset + ncrops > t->max_crops) return ERR_BATCH;
    const int S = t->cfg.image_size;
    std::vector<TrocrCrop> crops(ncrops);
    int rc;
    int rows_per_block = 8, lds_rows = 0;
    for (int i = 0; i < ncrops; ++i) {
        const int32_t* b = boxes_host + 5 * i;
        TrocrCrop& c = crops[i];
        c.frame = b[0]; c.x0 = b[1]; c.y0 = b[2]; c.w = b[3] - b[1]; c.h = b[4] - b[2];
        if (c.frame < 0 || c.frame >= n_frames || c.x0 < 0 || c.y0 < 0 || c.w <= 0 || c.h <= 0 || c.x0 + c.w > width || c.y0 + c.h > height)
            return ERR_GEOMETRY;
        if ((rc = trocr_axis(t, c.w, &c.xtab, &c.ksx)) || (rc = trocr_axis(t, c.h, &c.ytab, &c.ksy))) return rc;
    }
    // rows of the intermediate image a block of R output rows needs: R + the vertical filter's extent
    for (;; rows_per_block >>= 1) {
        lds_rows = 0;
        for (int i = 0; i < ncrops; ++i) {
            const int h = crops[i].h, ks = crops[i].ksy;
            const int span = std::min(h, (int)std::ceil((double)rows_per_block * h / S) + ks + 1);
            lds_rows = std::max(lds_rows, span);
        }
        if ((size_t)lds_rows * S * 3 <= (size_t)144 * 1024 || rows_per_block == 1) break;
    }
    if ((size_t)lds_rows * S * 3 > (size_t)144 * 1024) return ERR_CAPACITY;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = trocr_encoder_prologue(t, slot, s))) return rc;
    // the crop table travels through a pinned staging buffer of its own per slot (a pageable source would stall the host until the
    // stream drains, i.e. until the previous encoder pass is done); the slot's previous use of it -- two passes ago -- has long
    // completed, the wait below is there for correctness, not for timing (rows of one pass never overlap: one wait per pass)
    if (row_offset == 0 && t->slot_enc[slot]) VTD_HIP_CHECK(hipEventSynchronize(t->enc_done[slot]));
    std::memcpy(t->crops_pin[slot] + row_offset, crops.data(), (size_t)ncrops * sizeof(TrocrCrop));
    VTD_HIP_CHECK(hipMemcpyAsync(t->crops_dev + row_offset, t->crops_pin[slot] + row_offset, (size_t)ncrops * sizeof(TrocrCrop),
                                 hipMemcpyHostToDevice, s));
    return vtd_launch_trocr_resample(frames_dev, height, width, t->crops_dev + row_offset, t->pool,
                                     t->patches + (size_t)row_offset * t->NP * t->PK, ncrops, S, t->cfg.patch_size, rows_per_block, lds_rows, s);
}

// ViT encoder + cross-attention keys / values over the first `ncrops` staged rows of the slot.
int vtd_trocr_encode_staged_slot(vtd_trocr* t, int slot, int ncrops, vtd_stream stream) {
    if (!t || slot < 0 || slot >= t->n_slots) return ERR_ARG;
    if (!t->finalized) return ERR_NOT_FINALIZED;
    if (ncrops <= 0 || ncrops > t->max_crops) return ERR_BATCH;
    int rc = trocr_encoder_prologue(t, slot, (hipStream_t)stream);
    if (rc) return rc;
    return trocr_run_encoder(t, slot, ncrops, (hipStream_t)stream);
}

int vtd_trocr_encode_crops_slot(vtd_trocr* t, int slot, const uint8_t* frames_dev, int n_frames, int height, int width, const int32_t* boxes_host,
                                int ncrops, vtd_stream stream) {
    int rc = vtd_trocr_stage_crops_slot(t, slot, frames_dev, n_frames, height, width, boxes_host, ncrops, 0, stream);
    return rc ? rc : vtd_trocr_encode_staged_slot(t, slot, ncrops, stream);
}

int vtd_trocr_encode_crops(vtd_trocr* t, const uint8_t* frames_dev, int n_frames, int height, int width, const int32_t* boxes_host, int ncrops,
                           vtd_stream stream) {
    return vtd_trocr_encode_crops_slot(t, 0, frames_dev, n_frames, height, width, boxes_host, ncrops, stream);
}

int vtd_trocr_encode_pixels_slot(vtd_trocr* t, int slot, const float* pixel_values_dev, int ncrops, vtd_stream stream) {
    if (!t || !pixel_values_dev || slot < 0 || slot >= t->n_slots) return ERR_ARG;
    if (!t->finalized) return ERR_NOT_FINALIZED;
    if (ncrops <= 0 || ncrops > t->max_crops) return ERR_BATCH;
    int rc = trocr_encoder_prologue(t, slot, (hipStream_t)stream);
    if (rc) return rc;
    if ((rc = vtd_launch_trocr_pixels(pixel_values_dev, t->patches, ncrops, t->cfg.image_size, t->cfg.patch_size, (hipStream_t)stream))) return rc;
    return trocr_run_encoder(t, slot, ncrops, (hipStream_t)stream);
}

int vtd_trocr_encode_pixels(vtd_trocr* t, const float* pixel_values_dev, int ncrops, vtd_stream stream) {
    return vtd_trocr_encode_pixels_slot(t, 0, pixel_values_dev, ncrops, stream);
}

int vtd_trocr_num_slots(const vtd_trocr* t) { return t ? t->n_slots : 0; }

// Greedy decode of the crops last encoded into `slot` (GenerationMixin greedy search, text_recognizer.py:58 max_length = 50).
//
// Every kernel of a step works on the LIVE rows: once a row has emitted </s> it leaves the list (dec_advance) and costs nothing any
// more -- the reference pads such rows and keeps computing them; the ids it returns are the same.  The live count is exact on the
// device (every kernel reads it) and lags by up to kLag steps on the host, where it is an upper bound for the launch geometry and,
// at zero, the stop test: the host never waits for the step it is enqueueing, only for the one kLag steps back, so the GPU always has
// work queued.  Teacher forcing and logit capture index rows by crop, so they keep the full list (compaction off).
int vtd_trocr_generate_slot(vtd_trocr* t, int slot, int ncrops, int max_length, const int32_t* forced_ids_dev, int forced_len, int32_t* ids_dev,
                            float* logits_dev, vtd_stream stream) {
    if (!t || !ids_dev || slot < 0 || slot >= t->n_slots) return ERR_ARG;
    if (!t->finalized) return ERR_NOT_FINALIZED;
    if (ncrops <= 0 || ncrops > t->max_crops) return ERR_BATCH;
    const vtd_trocr_config& c = t->cfg;
    if (max_length < 2 || max_length > c.max_length || (forced_ids_dev && (forced_len < 2 || forced_len > max_length))) return ERR_ARG;
    if (!t->slot_enc[slot]) return ERR_ARG;   // nothing encoded into this slot yet
    hipStream_t s = (hipStream_t)stream;
    const int D = c.dec_hidden, DF = c.dec_ffn, V = c.vocab_size, T = t->T, n = ncrops, L = c.max_length;
    constexpr int kLag = 2;
    int rc;
    // the previous decode on this handle has left the host word alone (its last dec_advance has run) before this one starts using it
    if (t->dec_used) VTD_HIP_CHECK(hipEventSynchronize(t->dec_free));
    VTD_HIP_CHECK(hipStreamWaitEvent(s, t->enc_done[slot], 0));
    if (t->dec_used) VTD_HIP_CHECK(hipStreamWaitEvent(s, t->dec_free, 0));
    if ((rc = vtd_launch_dec_init(ids_dev, max_length, t->done, t->active, t->n_rows, n, c.decoder_start_token_id, c.pad_token_id, s))) return rc;
    const bool compact = !forced_ids_dev && !logits_dev && !(std::getenv("VTD_TROCR_COMPACT") && std::getenv("VTD_TROCR_COMPACT")[0] == '0');
    const int steps = (forced_ids_dev ? forced_len : max_length) - 1;
    const int64_t slab = (int64_t)t->rows_pad * D;
    // split-K of the N = D projections (their 2-D grid alone would leave most CUs idle and a workgroup's K walk sets the launch's
    // latency): slabs summed by the LayerNorm that follows.  A function of K ONLY -- never of the live row count, which the host knows
    // with a lag: the summation order of every output is then the same in every run (bitwise repeatable).
    auto pick_split = [&](int K) {
        int ks = 1;
        while (ks < kDecSplitMax && K / ks > 256 && K % (ks * 2 * 128) == 0) ks *= 2;
        return ks;
    };
    const int ks_d = pick_split(D), ks_f = pick_split(DF);
    int step = 0;
    // (the step loop as a callable: whatever it returns, the events that later passes order themselves by are recorded below -- a
    // failed launch must not leave the next encoder pass / decode waiting on an event that is never recorded)
    auto run_steps = [&]() -> int {
    for (; step < steps; ++step) {
        // live rows after step - kLag (its dec_advance wrote word step - kLag): an upper bound for this step, and the same
        // number in every run whatever the timing
        int m = n;
        if (step >= kLag) {
            VTD_HIP_CHECK(hipEventSynchronize(t->step_ev[(step - kLag) % 3]));
            m = ((volatile int*)t->host_rows)[step - kLag];
        }
        if (m <= 0) break;
        if (!compact) m = n;   // the list keeps every row in place: the count is only the stop test
        if ((rc = vtd_launch_dec_ln(t->dstream, t->d16, nullptr, 0, 0, nullptr, t->ln_emb.g, t->ln_emb.b, t->n_rows, m, D, c.dec_ln_eps, t->embed,
                                    t->pos_dec, ids_dev, t->active, max_length, step, step, V, s)))
            return rc;
        for (int i = 0; i < c.dec_layers; ++i) {
            TrocrDecLayer& l = t->dec[i];
            // self-attention: q | k | v in one projection; the attention kernel files k / v into the caches
            if ((rc = vtd_launch_dec_gemm(t->d16, D, l.sqkv.w, l.sqkv.bias, t->qkv16, 3 * D, 0, m, t->n_rows, 3 * D, D, 1, 1, 0, s))) return rc;
            if ((rc = vtd_launch_dec_attn(1, t->qkv16, 3 * D, l.kcache, l.vcache, (int64_t)L * D, step + 1, D, t->datt16, t->active, t->n_rows, m,
                                          c.dec_heads, s)))
                return rc;
            if ((rc = vtd_launch_dec_gemm(t->datt16, D, l.so.w, nullptr, t->slabs, D, slab, m, t->n_rows, D, D, ks_d, 4, 0, s))) return rc;
            if ((rc = vtd_launch_dec_ln(t->dstream, t->d16, t->slabs, slab, ks_d, l.so.bias, l.ln_self.g, l.ln_self.b, t->n_rows, m, D, c.dec_ln_eps,
                                        nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0, s)))
                return rc;
            // cross-attention on the encoder keys / values of the slot
            if ((rc = vtd_launch_dec_gemm(t->d16, D, l.cq.w, l.cq.bias, t->q16, D, 0, m, t->n_rows, D, D, 1, 1, 0, s))) return rc;
            hipEvent_t pe0 = nullptr, pe1 = nullptr;
            if ((t->prof_mode & 1) && i == 0) {
                if (t->prof_used == t->prof_ev.size()) {
                    hipEvent_t a, b;
                    VTD_HIP_CHECK(hipEventCreate(&a));
                    VTD_HIP_CHECK(hipEventCreate(&b));
                    t->prof_ev.push_back({a, b});
                    t->prof_rows.push_back({0, 0});
                }
                pe0 = t->prof_ev[t->prof_used].first; pe1 = t->prof_ev[t->prof_used].second;
                t->prof_rows[t->prof_used] = {step, n};
                ++t->prof_used;
                VTD_HIP_CHECK(hipEventRecord(pe0, s));
            }
            if (t->xattn) {
                // q' = q Wk_h per head -> attention over the raw encoder states (the bracketed, HBM-bound launch) -> value projection
                if ((rc = vtd_launch_dec_xq(t->q16, D, l.wkt, t->qp16, t->n_rows, m, c.dec_heads, c.enc_hidden, s))) return rc;
                if (pe0) VTD_HIP_CHECK(hipEventRecord(pe0, s));   // (bracket the attention alone)
                if ((rc = vtd_launch_dec_xattn(t->qp16, t->enc16[slot], t->cp16, t->active, t->n_rows, m, c.dec_heads, T, c.enc_hidden, s))) return rc;
                if (pe1) VTD_HIP_CHECK(hipEventRecord(pe1, s));
                if ((rc = vtd_launch_dec_xv(t->cp16, l.wv16, l.bv, t->datt16, t->n_rows, m, c.dec_heads, c.enc_hidden, D, s))) return rc;
            } else {
            if ((rc = vtd_launch_dec_attn(0, t->q16, D, l.ck_buf[slot], l.cv_buf[slot], (int64_t)T * D, T, D, t->datt16, t->active, t->n_rows, m,
                                          c.dec_heads, s)))
                return rc;
            if (pe1) VTD_HIP_CHECK(hipEventRecord(pe1, s));
            }
            if ((rc = vtd_launch_dec_gemm(t->datt16, D, l.co.w, nullptr, t->slabs, D, slab, m, t->n_rows, D, D, ks_d, 4, 0, s))) return rc;
            if ((rc = vtd_launch_dec_ln(t->dstream, t->d16, t->slabs, slab, ks_d, l.co.bias, l.ln_cross.g, l.ln_cross.b, t->n_rows, m, D, c.dec_ln_eps,
                                        nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0, s)))
                return rc;
            // feed-forward
            if ((rc = vtd_launch_dec_gemm(t->d16, D, l.fc1.w, l.fc1.bias, t->dffn16, DF, 0, m, t->n_rows, DF, D, 1, 1 | 2, 0, s))) return rc;
            if ((rc = vtd_launch_dec_gemm(t->dffn16, DF, l.fc2.w, nullptr, t->slabs, D, slab, m, t->n_rows, D, DF, ks_f, 4, 0, s))) return rc;
            if ((rc = vtd_launch_dec_ln(t->dstream, t->d16, t->slabs, slab, ks_f, l.fc2.bias, l.ln_final.g, l.ln_final.b, t->n_rows, m, D, c.dec_ln_eps,
                                        nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0, s)))
                return rc;
        }
        float* lg = logits_dev ? logits_dev + (size_t)step * t->vld : t->logits;
        const int64_t ld = logits_dev ? (int64_t)(max_length - 1) * t->vld : t->vld;
        if (ld > 0x7fffffff) return ERR_CAPACITY;
        if ((rc = vtd_launch_dec_gemm(t->d16, D, t->lm_head.w, t->lm_head.bias, lg, (int)ld, 0, m, t->n_rows, V, D, 1, 0, 1, s))) return rc;
        if ((rc = vtd_launch_dec_argmax(lg, ld, V, t->best_tok, t->n_rows, m, s))) return rc;
        if ((rc = vtd_launch_dec_advance(t->best_tok, ids_dev, max_length, step + 1, t->done, t->active, t->n_rows, t->host_rows + step, forced_ids_dev,
                                         forced_len, forced_len, c.eos_token_id, c.pad_token_id, compact ? 1 : 0, s)))
            return rc;
        VTD_HIP_CHECK(hipEventRecord(t->step_ev[step % 3], s));
    }
    return 0;
    };
    const int steps_rc = run_steps();
    t->last_steps = step;
    if (steps_rc) {
        (void)hipEventRecord(t->dec_done[slot], s);
        (void)hipEventRecord(t->dec_free, s);
        t->slot_dec[slot] = true;
        t->dec_used = true;
        return steps_rc;
    }
    if (t->prof_mode & 1) {   // measurement only: wait for the call and read the exact live rows of the bracketed launches off the ring
        VTD_HIP_CHECK(hipStreamSynchronize(s));
        t->prof_exact.resize(t->prof_ev.size(), 0);
        for (size_t i = 0; i < t->prof_used; ++i)
            if (t->prof_rows[i].second == n && t->prof_rows[i].first >= 0) {
                const int st = t->prof_rows[i].first;
                t->prof_exact[i] = (st == 0 || !compact) ? n : t->host_rows[st - 1];
                t->prof_rows[i].first = -1;   // resolved
            }
    }
    VTD_HIP_CHECK(hipEventRecord(t->dec_done[slot], s));
    VTD_HIP_CHECK(hipEventRecord(t->dec_free, s));
    t->slot_dec[slot] = true;
    t->dec_used = true;
    return 0;
}

int vtd_trocr_generate(vtd_trocr* t, int ncrops, int max_length, const int32_t* forced_ids_dev, int forced_len, int32_t* ids_dev, float* logits_dev,
                       vtd_stream stream) {
    return vtd_trocr_generate_slot(t, 0, ncrops, max_length, forced_ids_dev, forced_len, ids_dev, logits_dev, stream);
}

int vtd_trocr_last_steps(const vtd_trocr* t) { return t ? t->last_steps : 0; }

// Profiling of the decoder's dominant launch, the cross-attention (HBM-bound read of the encoder keys / values): mode 1 brackets the
// launch of decoder layer 0 of every step with HIP events on the decode stream; vtd_trocr_get_profile sums them up (and resets):
// total time, launches, and the live rows those launches were sized for (an upper bound of the rows they read).
int vtd_trocr_set_profiling(vtd_trocr* t, int mode) {
    if (!t) return ERR_ARG;
    t->prof_mode = mode;
    t->prof_used = 0;
    t->gprof_used = 0;
    return 0;
}

// Mode bit 1: every dense_gemm_kernel launch of the encoder pass (dense layers + the cross-attention key / value projections) is
// bracketed with HIP events on the stream it is launched on; returns their summed time, count and executed FLOPs (2 M N K), then resets.
int vtd_trocr_get_gemm_profile(vtd_trocr* t, double* total_ms, int64_t* launches, double* total_flops, vtd_stream stream) {
    if (!t || !total_ms || !launches || !total_flops) return ERR_ARG;
    VTD_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    *total_ms = 0.0; *launches = 0; *total_flops = 0.0;
    for (size_t i = 0; i < t->gprof_used; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, t->gprof_ev[i].first, t->gprof_ev[i].second) != hipSuccess) continue;
        *total_ms += ms; *launches += 1; *total_flops += t->gprof_flops[i];
    }
    t->gprof_used = 0;
    return 0;
}

int vtd_trocr_get_profile(vtd_trocr* t, double* total_ms, int64_t* launches, int64_t* row_launches, vtd_stream stream) {
    if (!t || !total_ms || !launches || !row_launches) return ERR_ARG;
    VTD_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    *total_ms = 0.0; *launches = 0; *row_launches = 0;
    for (size_t i = 0; i < t->prof_used; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, t->prof_ev[i].first, t->prof_ev[i].second) != hipSuccess) continue;
        *total_ms += ms; *launches += 1; *row_launches += t->prof_exact[i];
    }
    t->prof_used = 0;
    return 0;
}

int vtd_trocr_read_tap(vtd_trocr* t, const char* name, int ncrops, float* host_out, int64_t capacity, vtd_stream stream) {
    if (!t || !name || !host_out) return ERR_ARG;
    if (!t->finalized) return ERR_NOT_FINALIZED;
    if (ncrops <= 0 || ncrops > t->max_crops) return ERR_BATCH;
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return -(int)e;
    const std::string nm = name;
    if (nm == "encoder") {  // last_hidden_state [n][T][C]
        const int64_t need = (int64_t)ncrops * t->T * t->cfg.enc_hidden;
        if (capacity < need) return ERR_CAPACITY;
        e = hipMemcpy(host_out, t->enc_out32, need * sizeof(float), hipMemcpyDeviceToHost);
        return e == hipSuccess ? 0 : -(int)e;
    }
    if (nm == "pixel_values") {  // [n][3][S][S], undone from the patch-major fp16 layout
        const int S = t->cfg.image_size, P = t->cfg.patch_size, pw = S / P;
        const int64_t need = (int64_t)ncrops * 3 * S * S;
        if (capacity < need) return ERR_CAPACITY;
        std::vector<half_t> tmp((size_t)need);
        e = hipMemcpy(tmp.data(), t->patches, (size_t)need * sizeof(half_t), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return -(int)e;
        for (int64_t b = 0; b < ncrops; ++b)
            for (int ch = 0; ch < 3; ++ch)
                for (int y = 0; y < S; ++y)
                    for (int x = 0; x < S; ++x)
                        host_out[((b * 3 + ch) * S + y) * S + x] =
                            (float)tmp[(size_t)((b * pw * pw + (y / P) * pw + x / P) * (3 * P * P) + ch * P * P + (y % P) * P + x % P)];
        return 0;
    }
    return ERR_UNKNOWN_KEY;
}

int vtd_trocr_encoder_tokens(const vtd_trocr* t) { return t && t->finalized ? t->T : 0; }
int vtd_trocr_logits_stride(const vtd_trocr* t) { return t && t->finalized ? t->vld : 0; }
int64_t vtd_trocr_macs_per_crop(const vtd_trocr* t) { return t ? t->macs : 0; }

int vtd_trocr_set_tuning(vtd_trocr* t, const char* table_text) {
    if (!t) return ERR_ARG;
    int rc = set_tuning_text(t, table_text);
    if (!rc) t->tuned.clear();   // only encoder-pass launch slots resolve through the table now (the decoder chain has no variants)
    return rc;
}
int64_t vtd_trocr_get_tuning(const vtd_trocr* t, char* buf, int64_t capacity) { return get_tuning_text(t, buf, capacity); }
int vtd_trocr_tuning_measured(const vtd_trocr* t) { return t && t->tuning_measured ? 1 : 0; }

}  // extern "C"
