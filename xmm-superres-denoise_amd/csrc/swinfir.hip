// swinfir.hip -- the reference's SwinFIR super-resolution network (models/transformer/swinfir.py:120-441 with the Swin blocks of
// modules.py), FORWARD ONLY (eval mode: DropPath and Dropout are identities), in exact fp32.
//
// The GEMM (Linear / 1x1 / 3x3 conv with its epilogues), the (shifted-)window attention, the LayerNorm and the weight packing are the
// kernels of sw_kernels.h, which also states the arithmetic rules and the token-major layout; this file adds the FourierUnit's FFT,
// whose butterflies are fp32 FMAs on the vector ALUs in a fixed order, and the network.  The NHWC view of a token-major map is what
// PatchUnEmbed / PatchEmbed (modules.py:423-500) turn into NCHW and back, so the convs of the SFB block, the head and the tail read
// and write it through their addressing; only the network input and output are NCHW.
// The opt-in math mode bf16x6 (xsd_swinfir_set_math) runs the GEMMs on sw_gemm_s3x.h's kernel instead; attention, LayerNorm and the
// FFT stay exact fp32 in both modes.
//
// The FFT passes (sw_fft_kernel, its launcher, the twiddle table) are sw_fft.h's.
#include "sw_kernels.h"
#include "sw_gemm_s3x.h"
#include "sw_fft.h"

namespace {

struct Layer {
    std::vector<SBlk> blks;
    int heads;
    Lin s0, s2, c1, fu, c2, fus, conv1;      // SFB: S.body.0 / .2, F.conv1.0, F.fu.conv_layer, F.conv2, fusion; 1conv: conv
};

} // namespace

struct xsd_swinfir : SwBase {
    xsd_swinfir_config cfg;
    int C2 = 0;
    bool clamped = false;
    std::vector<Layer> layers;
    float *Y1 = nullptr, *S1 = nullptr, *S2 = nullptr;
    float2* tw = nullptr;             // roots of unity for H, then for W (device)
    int twH = 0, twW = 0;

    ~xsd_swinfir() { if (tw) xsd::dev_free(tw); }
};

namespace {

// the reference's registration order (swinfir.py:267-401; modules.py RSTB / BasicLayer / SwinTransformerBlock / WindowAttention / Mlp)
void layout(xsd_swinfir* r)
{
    const auto& c = r->cfg;
    const int E = r->E, side = 2 * r->ws - 1;
    long long off = 0;
    lin(r->first_l, off, E, c.in_chans, 9, true);
    if (c.patch_norm) { r->pen_w = add(off, E); r->pen_b = add(off, E); }
    for (int li = 0; li < c.num_layers; ++li) {
        Layer L;
        L.heads = c.num_heads[li];
        for (int j = 0; j < c.depths[li]; ++j) {
            SBlk k{};
            k.shift = (j % 2 == 0 || r->clamped) ? 0 : c.window_size / 2;      // BasicLayer (modules.py:552)
            k.n1w = add(off, E); k.n1b = add(off, E);
            k.table = add(off, (long long)side * side * L.heads);
            lin(k.qkv, off, 3 * E, E, 1, c.qkv_bias != 0);
            lin(k.proj, off, E, E, 1, true);
            k.n2w = add(off, E); k.n2b = add(off, E);
            lin(k.fc1, off, r->hid, E, 1, true);
            lin(k.fc2, off, E, r->hid, 1, true);
            L.blks.push_back(k);
        }
        if (c.resi_connection == 0) {
            lin(L.s0, off, E, E, 9, true);
            lin(L.s2, off, E, E, 9, true);
            lin(L.c1, off, r->C2, E, 1, true);
            lin(L.fu, off, 2 * r->C2, 2 * r->C2, 1, true);
            lin(L.c2, off, E, r->C2, 1, true);
            lin(L.fus, off, E, 2 * E, 1, true);
        } else {
            lin(L.conv1, off, E, E, 9, true);
        }
        r->layers.push_back(L);
    }
    r->norm_w = add(off, E); r->norm_b = add(off, E);
    lin(r->after, off, E, E, 9, true);
    lin(r->before, off, r->nfeat, E, 9, true);
    const int f = up_factor(c.upscale);
    for (int s = 0; s < up_stages(c.upscale); ++s) {
        Lin u;
        lin(u, off, f * f * r->nfeat, r->nfeat, 9, true);
        r->ups.push_back(u);
    }
    lin(r->last, off, c.in_chans, r->nfeat, 9, true);
    r->nparams = off;
    r->lins.push_back(&r->first_l);
    for (auto& L : r->layers) {
        for (auto& k : L.blks)
            for (Lin* p : {&k.qkv, &k.proj, &k.fc1, &k.fc2}) r->lins.push_back(p);
        for (Lin* p : {&L.s0, &L.s2, &L.c1, &L.fu, &L.c2, &L.fus, &L.conv1})
            if (p->cout) r->lins.push_back(p);
    }
    for (Lin* p : {&r->after, &r->before}) r->lins.push_back(p);
    for (auto& u : r->ups) r->lins.push_back(&u);
    r->lins.push_back(&r->last);
    long long t = 0;
    for (Lin* p : r->lins) p->t = add(t, (long long)p->cout * p->cin * p->taps);
    r->wt_floats = t;
}

// workspace of one (B, H, W) in floats; with `assign` set, also the pointers into r->ws_buf
long long plan_ws(xsd_swinfir* r, int B, int H, int W, bool assign)
{
    const long long M = (long long)B * H * W, E = r->E, Ms = (long long)B * H * (W / 2 + 1);
    const long long up = (long long)r->cfg.upscale * r->cfg.upscale;
    const long long sizes[11] = {M * E, M * E, M * std::max({3 * E, (long long)r->hid, 2 * E}), M * E, M * r->C2, Ms * 2 * r->C2,
                                 Ms * 2 * r->C2, M * r->nfeat, M * up * r->nfeat, M * up * r->nfeat, M * E};
    float** ptrs[11] = {&r->XF, &r->X, &r->A, &r->O, &r->Y1, &r->S1, &r->S2, &r->V, &r->U0, &r->U1, &r->R0};
    long long off = 0;
    for (int i = 0; i < 11; ++i) {
        if (assign) *ptrs[i] = (float*)r->ws_buf + off;
        off += (std::max(sizes[i], 1ll) + 63) / 64 * 64;        // 256-B aligned
    }
    return off;
}

int set_twiddles(xsd_swinfir* r, int H, int W)
{
    if (r->twH == H && r->twW == W) return XSD_OK;
    std::vector<float2> t((size_t)H + W);
    fft_twiddles(H, W, t.data());                         // sw_fft.h
    // The one place that pairs the planned shape with the table: a plan (r->B / H / W) is valid only for the table it was made with, so
    // giving the table up clears it, for the forward and for xsd_swinfir_test_fft alike.  A forward at the shape held so far must not
    // skip its plan and read a table that is gone (a smaller shape fits the held workspace, so grow_ws leaves the plan alone, and a
    // refused allocation below would return with it set).
    if (r->tw) { hipDeviceSynchronize(); xsd::dev_free(r->tw); r->tw = nullptr; r->twH = r->twW = 0; r->B = r->H = r->W = 0; }
    if (xsd::dev_alloc((void**)&r->tw, sizeof(float2) * t.size()) != hipSuccess) {
        (void)hipGetLastError();
        return rfail(XSD_ERR_NOMEM, "SwinFIR: twiddle table allocation failed");
    }
    // the upload goes to stream 0, the FFT passes that read the table to the caller's stream, which stream 0 does not order when it is
    // non-blocking: the table is on the device before the passes are enqueued
    if (hipMemcpy(r->tw, t.data(), sizeof(float2) * t.size(), hipMemcpyHostToDevice) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
        return rfail(XSD_ERR_HIP, "SwinFIR: twiddle table upload failed");
    r->twH = H; r->twW = W;
    return XSD_OK;
}

const char* resi_name(int u)
{
    switch (u) { case 0: return "SFB"; case 1: return "1conv"; case 2: return "HSFB"; default: return "identity"; }
}

} // namespace

extern "C" {

int xsd_swinfir_fft_supported(int n)
{
    std::vector<int> rad;
    return n >= 1 && n <= FFT_MAXN && radices(n, rad) ? 1 : 0;
}

int xsd_swinfir_create(const xsd_swinfir_config* cfg, xsd_swinfir** out)
{
    if (!cfg || !out) return rfail(XSD_ERR_ARG, "null argument");
    const auto& c = *cfg;
    if (c.ape) return rfail(XSD_ERR_ARG, "SwinFIR: ape=True (absolute position embedding) is not supported by the MI355X engine");
    if (c.upsampler != 0)
        return rfail(XSD_ERR_ARG, "SwinFIR: upsampler %s is not supported by the MI355X engine (only \"pixelshuffle\")", upsampler_name(c.upsampler));
    if (c.resi_connection != 0 && c.resi_connection != 1)
        return rfail(XSD_ERR_ARG, "SwinFIR: resi_connection %s is not supported by the MI355X engine (only \"SFB\" and \"1conv\")",
                     resi_name(c.resi_connection));
    if (int rc = check_dims(c, "SwinFIR")) return rc;
    const int res = std::min(c.img_size[0] / c.patch_size[0], c.img_size[1] / c.patch_size[1]);
    const bool clamped = res <= c.window_size;                      // SwinTransformerBlock.__init__ (modules.py:236-239): no shift then
    const int ws = clamped ? res : c.window_size;
    if (ws < 1) return rfail(XSD_ERR_ARG, "SwinFIR: img_size // patch_size is 0");
    if (ws > 16) return rfail(XSD_ERR_ARG, "SwinFIR: an effective window of %d exceeds the engine's 16 (256 tokens per window)", ws);
    if (int rc = check_layers(c, "SwinFIR")) return rc;
    if (c.resi_connection == 0 && c.embed_dim < 2) return rfail(XSD_ERR_ARG, "SwinFIR: SFB needs embed_dim >= 2");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return rfail(XSD_ERR_HIP, "no HIP device available");
    xsd_swinfir* r = new xsd_swinfir();
    r->cfg = c;
    r->E = c.embed_dim;
    r->hid = (int)(c.embed_dim * c.mlp_ratio);
    r->C2 = c.embed_dim / 2;
    r->ws = ws;
    r->clamped = clamped;
    layout(r);
    std::vector<float> mean(c.in_chans, 0.f);
    if (c.in_chans == 3) { mean[0] = 0.3014f; mean[1] = 0.3152f; mean[2] = 0.3094f; }   // swinfir.py:319-323
    if (int rc = alloc_weights(r, "SwinFIR", mean)) {
        delete r;
        return rc;
    }
    *out = r;
    return XSD_OK;
}

void xsd_swinfir_destroy(xsd_swinfir* r) { delete r; }

int64_t xsd_swinfir_param_count(const xsd_swinfir* r) { return r ? r->nparams : -1; }

int xsd_swinfir_pack_weights(xsd_swinfir* r, const float* dev_params, void* stream)
{
    return pack_weights(r, "SwinFIR", dev_params, stream);
}

int xsd_swinfir_set_math(xsd_swinfir* r, int mode) { return set_math(r, "SwinFIR", mode); }

int xsd_swinfir_get_math(const xsd_swinfir* r) { return r ? r->math : -1; }

int xsd_swinfir_forward(xsd_swinfir* r, const float* dev_x, float* dev_y, int B, int H, int W, void* stream)
{
    if (!r || !dev_x || !dev_y) return rfail(XSD_ERR_ARG, "null argument");
    if (B < 1 || H < 1 || W < 1) return rfail(XSD_ERR_ARG, "bad shape %dx%dx%d", B, H, W);
    if (H % r->ws || W % r->ws)
        return rfail(XSD_ERR_ARG, "SwinFIR: H and W must be multiples of the window size %d (window_partition); got %d x %d", r->ws, H, W);
    if (r->cfg.resi_connection == 0)
        for (int n : {H, W})
            if (!xsd_swinfir_fft_supported(n))
                return rfail(XSD_ERR_ARG, "SwinFIR: FFT size %d is not supported (the FourierUnit needs H and W of at most %d whose prime factors are all "
                             "<= 13); got %d x %d", n, FFT_MAXN, H, W);
    const long long up = r->cfg.upscale;
    if ((long long)H * W * up * up > (1ll << 28)) return rfail(XSD_ERR_ARG, "SwinFIR: image of %d x %d pixels is too large", H, W);
    if (!r->packed) return rfail(XSD_ERR_STATE, "xsd_swinfir_pack_weights must be called before xsd_swinfir_forward");
    if (int rc = ready_math(r, "SwinFIR", (hipStream_t)stream)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (r->B != B || r->H != H || r->W != W) {
        int rc = grow_ws(r, "SwinFIR", plan_ws(r, B, H, W, false), B, H, W);
        if (rc) return rc;
        rc = set_twiddles(r, H, W);
        if (rc) return rc;
        plan_ws(r, B, H, W, true);
        r->B = B; r->H = H; r->W = W;
    }
    const auto& c = r->cfg;
    const int E = r->E, C2 = r->C2;
    const long long HW = (long long)H * W, M = B * HW, Ms = (long long)B * H * (W / 2 + 1);
    float* X = r->X;
    float* O = r->O;
    float* const XF = r->XF;
    const FftShape fs{B, H, W, C2, r->tw};
    const float* wt = r->wt;
    hipError_t e = hipSuccess;
#define SW(x) do { if ((e = (x)) != hipSuccess) return rfail(XSD_ERR_HIP, "SwinFIR forward: %s (%s:%d)", hipGetErrorString(e), __FILE__, __LINE__); } while (0)
    SW(head(s, r, dev_x, c.in_chans, (float)c.img_range, c.patch_norm != 0));        // swinfir.py:425-430, modules.py:455-461
    for (const Layer& L : r->layers) {
        // the RSTB's input: its `+ x` (swinfir.py:214-216) adds it after the blocks and the conv
        SW(hipMemcpyAsync(r->R0, X, sizeof(float) * M * E, hipMemcpyDeviceToDevice, s));
        for (const SBlk& k : L.blks) {
            SW(swin_block(s, r, k, X, O, B, H, W, L.heads, attn_scale(c.qk_scale, E / L.heads)));      // sw_kernels.h
        }
        if (c.resi_connection == 0) {
            // RSTB tail x = SFB(x) + RSTB input (swinfir.py:103-117, :214-216); CAT = [S | F] as the row halves of the A buffer
            float* CAT = r->A;
            GemmP p = gp_conv(X, B, H, W, E, wt + L.s0.t, E, PP(r, L.s0.b), O, E);
            p.act = ACT_LRELU; p.slope = 0.2f;
            SW(gemm(s, r, p));
            p = gp_conv(O, B, H, W, E, wt + L.s2.t, E, PP(r, L.s2.b), CAT, 2 * E);
            p.res = X; p.rbs = HW * E; p.rps = E;
            SW(gemm(s, r, p));
            p = gp_tok(X, M, E, E, wt + L.c1.t, C2, PP(r, L.c1.b), r->Y1, C2);
            p.act = ACT_LRELU; p.slope = 0.2f;
            SW(gemm(s, r, p));
            SW(fft(fs, s, F_R2C_ROWS, r->Y1, r->S1));
            SW(fft(fs, s, F_COLS_FWD, r->S1, r->S1));
            p = gp_tok(r->S1, Ms, 2 * C2, 2 * C2, wt + L.fu.t, 2 * C2, PP(r, L.fu.b), r->S2, 2 * C2);
            p.act = ACT_LRELU; p.slope = 0.2f;
            SW(gemm(s, r, p));
            SW(fft(fs, s, F_COLS_INV, r->S2, r->S2));
            SW(fft(fs, s, F_C2R_ROWS, r->S2, r->Y1));                                             // Y1 = x + fu(x)
            p = gp_tok(r->Y1, M, C2, C2, wt + L.c2.t, E, PP(r, L.c2.b), CAT + E, 2 * E);
            SW(gemm(s, r, p));
            p = gp_tok(CAT, M, 2 * E, 2 * E, wt + L.fus.t, E, PP(r, L.fus.b), X, E);
            p.res = r->R0; p.rbs = 0; p.rps = E;
            SW(gemm(s, r, p));
        } else {
            GemmP p = gp_conv(X, B, H, W, E, wt + L.conv1.t, E, PP(r, L.conv1.b), O, E);
            p.res = r->R0; p.rbs = HW * E; p.rps = E;
            SW(gemm(s, r, p));
            std::swap(X, O);
        }
    }
    // norm, conv_after_body + conv_first's output, then conv_before_upsample, Upsample, conv_last (swinfir.py:430-433)
    SW(ln(s, X, O, PP(r, r->norm_w), PP(r, r->norm_b), M, E));
    {
        GemmP p = gp_conv(O, B, H, W, E, wt + r->after.t, E, PP(r, r->after.b), X, E);
        p.res = XF; p.rbs = HW * E; p.rps = E;
        SW(gemm(s, r, p));
    }
    SW(tail(s, r, X, dev_y, c.in_chans, c.upscale, (float)c.img_range));
#undef SW
    return XSD_OK;
}

// the FourierUnit's transform pair on its own (tests): x [B][H][W][C2] real (token-major) -> spec [B][H][W/2+1][2 C2] = rfftn(ortho),
// and, with inverse set, spec -> x += irfftn(spec, s=(H, W), ortho).  Needs an engine for the twiddle table; takes no weights.
int xsd_swinfir_test_fft(xsd_swinfir* r, float* dev_x, float* dev_spec, int B, int H, int W, int C2, int inverse, void* stream)
{
    if (!r || !dev_x || !dev_spec) return rfail(XSD_ERR_ARG, "null argument");
    if (B < 1 || C2 < 1) return rfail(XSD_ERR_ARG, "bad shape");
    for (int n : {H, W})
        if (!xsd_swinfir_fft_supported(n))
            return rfail(XSD_ERR_ARG, "SwinFIR: FFT size %d is not supported (at most %d, prime factors <= 13)", n, FFT_MAXN);
    hipStream_t s = (hipStream_t)stream;
    if (r->twH != H || r->twW != W) {
        hipStreamSynchronize(s);
        int rc = set_twiddles(r, H, W);
        if (rc) return rc;              // (set_twiddles cleared the planned shape with the old table: the next forward plans again)
    }
    const FftShape fs{B, H, W, C2, r->tw};
    hipError_t e = inverse ? fft(fs, s, F_COLS_INV, dev_spec, dev_spec) : fft(fs, s, F_R2C_ROWS, dev_x, dev_spec);
    if (!e) e = inverse ? fft(fs, s, F_C2R_ROWS, dev_spec, dev_x) : fft(fs, s, F_COLS_FWD, dev_spec, dev_spec);
    if (e) return rfail(XSD_ERR_HIP, "SwinFIR FFT test: %s", hipGetErrorString(e));
    return XSD_OK;
}

int xsd_sw_test_gemm(const float* dev_a, const float* dev_w, const float* dev_bias, float* dev_y, int conv3, int B, int H, int W, int cin,
                     int N, int64_t ldy, int act, float slope, int math, void* stream)
{
    return test_gemm(dev_a, dev_w, dev_bias, dev_y, conv3, B, H, W, cin, N, ldy, act, slope, math, (hipStream_t)stream);
}

// One launch of this file's GEMM instances as the forwards describe theirs (tests): see include/xsd.h, xsd_sw_gemm_view.
int xsd_sw_test_gemm_view(const xsd_sw_gemm_view* view, void* stream) { return test_gemm_view(view, (hipStream_t)stream); }

// The shifted-window attention of both networks on its own (tests): see include/xsd.h, xsd_sw_test_attention.
int xsd_sw_test_attention(const float* dev_qkv, const float* dev_table, float* dev_out, int B, int H, int W, int C, int heads, int ws, int shift,
                          float scale, void* stream)
{
    if (!dev_qkv || !dev_table || !dev_out) return rfail(XSD_ERR_ARG, "null argument");
    if (B < 1 || H < 1 || W < 1) return rfail(XSD_ERR_ARG, "window attention test: bad shape %dx%dx%d", B, H, W);
    if (ws < 1 || ws > 16) return rfail(XSD_ERR_ARG, "window attention test: window size %d is outside [1, 16] (256 tokens per window)", ws);
    if (H % ws || W % ws)
        return rfail(XSD_ERR_ARG, "window attention test: H and W must be multiples of the window size %d; got %d x %d", ws, H, W);
    if (shift < 0 || shift >= ws) return rfail(XSD_ERR_ARG, "window attention test: shift %d is outside [0, window size %d)", shift, ws);
    if (heads < 1 || heads > 65535 || C < 1 || C % heads)
        return rfail(XSD_ERR_ARG, "window attention test: %d heads do not divide %d channels", heads, C);
    if (C / heads > 32) return rfail(XSD_ERR_ARG, "window attention test: head dim %d; the kernel takes at most 32", C / heads);
    if ((long long)B * (H / ws) * (W / ws) > 0x7fffffffll || (long long)B * H * W > (1ll << 28))
        return rfail(XSD_ERR_ARG, "window attention test: %d images of %d x %d tokens are too many", B, H, W);
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = attention(s, dev_qkv, dev_out, dev_table, B, H, W, C, heads, ws, shift, scale);
    hipStreamSynchronize(s);
    if (e) return rfail(XSD_ERR_HIP, "window attention test: %s", hipGetErrorString(e));
    return XSD_OK;
}

// The token LayerNorm of both networks on its own (tests): see include/xsd.h, xsd_sw_test_layernorm.
int xsd_sw_test_layernorm(const float* dev_x, const float* dev_w, const float* dev_b, float* dev_y, int64_t M, int C, void* stream)
{
    if (!dev_x || !dev_w || !dev_b || !dev_y) return rfail(XSD_ERR_ARG, "null argument");
    if (M < 1 || M > (1ll << 31)) return rfail(XSD_ERR_ARG, "LayerNorm test: %lld rows are outside [1, 2^31]", (long long)M);
    if (C < 1 || C > 4096) return rfail(XSD_ERR_ARG, "LayerNorm test: %d channels are outside [1, 4096]", C);
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = ln(s, dev_x, dev_y, dev_w, dev_b, M, C);
    hipStreamSynchronize(s);
    if (e) return rfail(XSD_ERR_HIP, "LayerNorm test: %s", hipGetErrorString(e));
    return XSD_OK;
}

} // extern "C"
