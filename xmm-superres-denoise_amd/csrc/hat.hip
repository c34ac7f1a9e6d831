// hat.hip -- the reference's HAT super-resolution network (models/transformer/hat.py:10-913), FORWARD ONLY (eval mode: DropPath and
// the dropouts are identities), in exact fp32, for upsampler "pixelshuffle".
//
// The GEMM (Linear / 1x1 / 3x3 conv with its GELU, LeakyReLU, residual, PixelShuffle and NCHW epilogues), the shifted-window attention
// of the HABs, the LayerNorm and the weight packing are the kernels HAT shares with SwinFIR (sw_kernels.h), as is the host code of the
// head, the MLP half block and the tail; this file adds what HAT has on top of them.  The same rules hold: every product an fp32 FMA,
// sums over K and all statistics carried in double, no float atomics, every reduction in a fixed order, so an image's output is
// bitwise independent of the batch it shares and of the run, and a NaN stays in its image.  The opt-in math mode bf16x6 (xsd_hat_set_math)
// runs the GEMMs on sw_gemm_s3x.h's kernel instead; everything in this file stays exact fp32 in both modes.
//
// Kernels (the first three and their launch code live in hat_kernels.h, which hat_ops.hip compiles too):
//   hat_ocab_kernel          the overlapping cross-attention of an OCAB (hat.py:326-391), one workgroup per (window, head): the ws^2
//                            queries of a window against the ow^2 keys / values of the overlapping window around it (ow = ws +
//                            int(ws overlap_ratio), stride ws, zero padding (ow - ws) / 2: nn.Unfold), read straight from the qkv token
//                            rows and written through the window-reverse addressing.  Keys outside the image are zero vectors that
//                            take part in the softmax with score = bias.  The bias is table[rpi_oca], the index computed here
//                            (hat.py:805-834, negative indices wrapping as torch's indexing wraps them).  The keys go through LDS in
//                            chunks of 64, twice: once for the row maxima, once for exp / sum / P V (no rescaling, a fixed order; the chunks' sums in double).
//   hat_pool_partial_kernel  the first stage of AdaptiveAvgPool2d(1) (hat.py:20): per image, channel and chunk of 256 pixels, a sum in double
//   hat_ca_kernel            one workgroup per image: the partial sums in chunk order -> the mean, then the squeeze MLP
//                            conv1x1 -> ReLU -> conv1x1 -> Sigmoid (hat.py:21-24)
//   hat_combine_kernel       x += (t * y[b, c]) * conv_scale (hat.py:29, :268), and with y null the plain x += t of the "identity" branches
#include "sw_kernels.h"
#include "sw_gemm_s3x.h"
#include "hat_kernels.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------
// combine
// ---------------------------------------------------------------------------------------------------------------
// x[i] += (t[i] * y[b][c]) * scale, i = (b HW + p) C + c; y null: x[i] += t[i] * scale
__global__ __launch_bounds__(256) void hat_combine_kernel(float* x, const float* t, const float* y, float scale, long long HWC, int C,
                                                          long long total)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    float v = t[i];
    if (y) v = v * y[(i / HWC) * C + (int)(i % C)];
    x[i] = x[i] + v * scale;
}

hipError_t combine(hipStream_t s, float* x, const float* t, const float* y, float scale, int B, long long HW, int C)
{
    const long long total = (long long)B * HW * C;
    hipLaunchKernelGGL(hat_combine_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, t, y, scale, HW * C, C, total);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
struct HBlk {                    // HAB (hat.py:141-271)
    long long n1w, n1b, table, n2w, n2b;
    Lin qkv, proj, c1, c2, sq1, sq2, fc1, fc2;     // conv_block.cab.0 / .2, cab.3.attention.1 / .3
    int shift;
};

struct OBlk {                    // OCAB (hat.py:274-396): its own parameter (the table) comes before its submodules'
    long long table, n1w, n1b, n2w, n2b;
    Lin qkv, proj, fc1, fc2;
};

struct HLayer {
    std::vector<HBlk> blks;
    OBlk oca;
    int heads;
    Lin conv;                    // "1conv"
};

} // namespace

struct xsd_hat : SwBase {
    xsd_hat_config cfg;
    int Cc = 0, Cs = 0, ow = 0;
    bool noshift = false;
    std::vector<HLayer> layers;
    float *T1 = nullptr, *T2 = nullptr, *YC = nullptr, *PART = nullptr;
};

namespace {

// the reference's registration order (hat.py:694-783; RHAG / AttenBlocks / HAB / WindowAttention / CAB / ChannelAttention / OCAB / Mlp)
void layout(xsd_hat* r)
{
    const auto& c = r->cfg;
    const int E = r->E, side = 2 * r->ws - 1, oside = r->ws + r->ow - 1;
    long long off = 0;
    lin(r->first_l, off, E, c.in_chans, 9, true);
    if (c.patch_norm) { r->pen_w = add(off, E); r->pen_b = add(off, E); }
    for (int li = 0; li < c.num_layers; ++li) {
        HLayer L;
        L.heads = c.num_heads[li];
        for (int j = 0; j < c.depths[li]; ++j) {
            HBlk k{};
            k.shift = (j % 2 == 0 || r->noshift) ? 0 : c.window_size / 2;       // AttenBlocks (hat.py:454), HAB (hat.py:186-189)
            k.n1w = add(off, E); k.n1b = add(off, E);
            k.table = add(off, (long long)side * side * L.heads);
            lin(k.qkv, off, 3 * E, E, 1, c.qkv_bias != 0);
            lin(k.proj, off, E, E, 1, true);
            lin(k.c1, off, r->Cc, E, 9, true);
            lin(k.c2, off, E, r->Cc, 9, true);
            lin(k.sq1, off, r->Cs, E, 1, true);
            lin(k.sq2, off, E, r->Cs, 1, true);
            k.n2w = add(off, E); k.n2b = add(off, E);
            lin(k.fc1, off, r->hid, E, 1, true);
            lin(k.fc2, off, E, r->hid, 1, true);
            L.blks.push_back(k);
        }
        OBlk& o = L.oca;
        o.table = add(off, (long long)oside * oside * L.heads);
        o.n1w = add(off, E); o.n1b = add(off, E);
        lin(o.qkv, off, 3 * E, E, 1, c.qkv_bias != 0);
        lin(o.proj, off, E, E, 1, true);
        o.n2w = add(off, E); o.n2b = add(off, E);
        lin(o.fc1, off, r->hid, E, 1, true);
        lin(o.fc2, off, E, r->hid, 1, true);
        if (c.resi_connection == 0) lin(L.conv, off, E, E, 9, true);
        r->layers.push_back(L);
    }
    r->norm_w = add(off, E); r->norm_b = add(off, E);
    if (c.resi_connection == 0) lin(r->after, off, E, E, 9, true);
    lin(r->before, off, r->nfeat, E, 9, true);
    const int f = up_factor(c.upscale);
    for (int s = 0; s < up_stages(c.upscale); ++s) {
        Lin u;
        lin(u, off, f * f * r->nfeat, r->nfeat, 9, true);
        r->ups.push_back(u);
    }
    lin(r->last, off, c.in_chans, r->nfeat, 9, true);
    r->nparams = off;
    // the weights the GEMM reads are packed to [taps][cin][cout]; the squeeze MLP reads its two 1x1 weights as stored
    r->lins.push_back(&r->first_l);
    for (auto& L : r->layers) {
        for (auto& k : L.blks)
            for (Lin* p : {&k.qkv, &k.proj, &k.c1, &k.c2, &k.fc1, &k.fc2}) r->lins.push_back(p);
        for (Lin* p : {&L.oca.qkv, &L.oca.proj, &L.oca.fc1, &L.oca.fc2}) r->lins.push_back(p);
        if (L.conv.cout) r->lins.push_back(&L.conv);
    }
    if (r->after.cout) r->lins.push_back(&r->after);
    r->lins.push_back(&r->before);
    for (auto& u : r->ups) r->lins.push_back(&u);
    r->lins.push_back(&r->last);
    long long t = 0;
    for (Lin* p : r->lins) p->t = add(t, (long long)p->cout * p->cin * p->taps);
    r->wt_floats = t;
}

// workspace of one (B, H, W) in floats; with `assign` set, also the pointers into r->ws_buf
long long plan_ws(xsd_hat* r, int B, int H, int W, bool assign)
{
    const long long HW = (long long)H * W, M = B * HW, E = r->E;
    const long long up = (long long)r->cfg.upscale * r->cfg.upscale;
    const long long sizes[12] = {M * E, M * E, M * std::max(3 * E, (long long)r->hid), M * E, M * r->Cc, M * E, M * r->nfeat,
                                 M * up * r->nfeat, M * up * r->nfeat, M * E, (long long)B * E, 2ll * B * pool_chunks(HW) * E};
    float** ptrs[12] = {&r->XF, &r->X, &r->A, &r->O, &r->T1, &r->T2, &r->V, &r->U0, &r->U1, &r->R0, &r->YC, &r->PART};
    long long off = 0;
    for (int i = 0; i < 12; ++i) {
        if (assign) *ptrs[i] = (float*)r->ws_buf + off;
        off += (std::max(sizes[i], 1ll) + 63) / 64 * 64;        // 256-B aligned
    }
    return off;
}

} // namespace

extern "C" {

int xsd_hat_create(const xsd_hat_config* cfg, xsd_hat** out)
{
    if (!cfg || !out) return rfail(XSD_ERR_ARG, "null argument");
    const auto& c = *cfg;
    if (c.ape) return rfail(XSD_ERR_ARG, "HAT: ape=True (absolute position embedding) is not supported by the MI355X engine");
    if (c.upsampler != 0)
        return rfail(XSD_ERR_ARG, "HAT: upsampler %s is not supported by the MI355X engine (only \"pixelshuffle\")", upsampler_name(c.upsampler));
    if (c.resi_connection != 0 && c.resi_connection != 1)
        return rfail(XSD_ERR_ARG, "HAT: this resi_connection is not supported (only \"1conv\" and \"identity\": the reference has no other branch)");
    if (int rc = check_dims(c, "HAT")) return rc;
    if (c.window_size > 16) return rfail(XSD_ERR_ARG, "HAT: window_size %d exceeds the engine's 16 (256 tokens per window)", c.window_size);
    const int res = std::min(c.img_size[0] / c.patch_size[0], c.img_size[1] / c.patch_size[1]);
    if (res < c.window_size)
        return rfail(XSD_ERR_ARG, "HAT: img_size // patch_size = %d is smaller than window_size %d (the reference's HAB clamps its window, its "
                     "index table does not follow, and its forward fails)", res, c.window_size);
    if (!(c.overlap_ratio >= 0) || c.overlap_ratio > 64) return rfail(XSD_ERR_ARG, "HAT: overlap_ratio %g is not supported", c.overlap_ratio);
    const int ext = (int)(c.window_size * c.overlap_ratio);
    if (ext % 2) return rfail(XSD_ERR_ARG, "HAT: int(window_size * overlap_ratio) = %d is odd (the reference's unfold then yields the wrong number of "
                              "windows)", ext);
    if (c.window_size + ext > OC_MAX_OW)
        return rfail(XSD_ERR_ARG, "HAT: an overlap window of %d exceeds the engine's %d", c.window_size + ext, OC_MAX_OW);
    {   // the largest index the reference's shift produces, ws (ws + ow), must lie inside the (ws + ow - 1)^2 table (window 1, no overlap: it does not)
        const int ow = c.window_size + ext, side = c.window_size + ow - 1;
        if (c.window_size * (c.window_size + ow) >= side * side)
            return rfail(XSD_ERR_ARG, "HAT: window_size %d with an overlap window of %d indexes past the OCAB's bias table in the reference", c.window_size, ow);
    }
    if (c.compress_ratio < 1 || c.embed_dim / c.compress_ratio < 1)
        return rfail(XSD_ERR_ARG, "HAT: embed_dim // compress_ratio must be at least 1 (embed_dim %d, compress_ratio %d)", c.embed_dim, c.compress_ratio);
    if (c.squeeze_factor < 1 || c.embed_dim / c.squeeze_factor < 1)
        return rfail(XSD_ERR_ARG, "HAT: embed_dim // squeeze_factor must be at least 1 (embed_dim %d, squeeze_factor %d)", c.embed_dim, c.squeeze_factor);
    if (int rc = check_layers(c, "HAT")) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return rfail(XSD_ERR_HIP, "no HIP device available");
    xsd_hat* r = new xsd_hat();
    r->cfg = c;
    r->E = c.embed_dim;
    r->hid = (int)(c.embed_dim * c.mlp_ratio);
    r->Cc = c.embed_dim / c.compress_ratio;
    r->Cs = c.embed_dim / c.squeeze_factor;
    r->ws = c.window_size;
    r->ow = c.window_size + ext;
    r->noshift = res <= c.window_size;                       // HAB.__init__ (hat.py:186-189), decided at construction
    layout(r);
    std::vector<float> mean(c.in_chans, 0.f);
    if (c.in_chans == 3) { mean[0] = 0.4488f; mean[1] = 0.4371f; mean[2] = 0.4040f; }   // hat.py:680-684
    if (int rc = alloc_weights(r, "HAT", mean)) {
        delete r;
        return rc;
    }
    *out = r;
    return XSD_OK;
}

void xsd_hat_destroy(xsd_hat* r) { delete r; }

int64_t xsd_hat_param_count(const xsd_hat* r) { return r ? r->nparams : -1; }

int xsd_hat_pack_weights(xsd_hat* r, const float* dev_params, void* stream)
{
    return pack_weights(r, "HAT", dev_params, stream);
}

int xsd_hat_set_math(xsd_hat* r, int mode) { return set_math(r, "HAT", mode); }

int xsd_hat_get_math(const xsd_hat* r) { return r ? r->math : -1; }

int xsd_hat_forward(xsd_hat* r, const float* dev_x, float* dev_y, int B, int H, int W, void* stream)
{
    if (!r || !dev_x || !dev_y) return rfail(XSD_ERR_ARG, "null argument");
    if (B < 1 || H < 1 || W < 1) return rfail(XSD_ERR_ARG, "bad shape %dx%dx%d", B, H, W);
    if (B > 65535) return rfail(XSD_ERR_ARG, "HAT: at most 65535 images per call (got %d)", B);
    if (H % r->ws || W % r->ws)
        return rfail(XSD_ERR_ARG, "HAT: H and W must be multiples of the window size %d (window_partition; the reference does not pad); got %d x %d",
                     r->ws, H, W);
    const long long up = r->cfg.upscale;
    if ((long long)H * W * up * up > (1ll << 28)) return rfail(XSD_ERR_ARG, "HAT: image of %d x %d pixels is too large", H, W);
    if (!r->packed) return rfail(XSD_ERR_STATE, "xsd_hat_pack_weights must be called before xsd_hat_forward");
    if (int rc = ready_math(r, "HAT", (hipStream_t)stream)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (r->B != B || r->H != H || r->W != W) {
        int rc = grow_ws(r, "HAT", plan_ws(r, B, H, W, false), B, H, W);
        if (rc) return rc;
        plan_ws(r, B, H, W, true);
        r->B = B; r->H = H; r->W = W;
    }
    const auto& c = r->cfg;
    const int E = r->E;
    const long long HW = (long long)H * W, M = B * HW;
    float* X = r->X;
    float* O = r->O;
    float* const XF = r->XF;
    double* const PART = (double*)r->PART;
    const float* wt = r->wt;
    hipError_t e = hipSuccess;
#define HT(x) do { if ((e = (x)) != hipSuccess) return rfail(XSD_ERR_HIP, "HAT forward: %s (%s:%d)", hipGetErrorString(e), __FILE__, __LINE__); } while (0)
    HT(head(s, r, dev_x, c.in_chans, (float)c.img_range, c.patch_norm != 0));          // hat.py:901-906, :887
    for (const HLayer& L : r->layers) {
        // the RHAG's input: its `+ x` (hat.py:603-611) adds it after the blocks and the conv
        HT(hipMemcpyAsync(r->R0, X, sizeof(float) * M * E, hipMemcpyDeviceToDevice, s));
        for (const HBlk& k : L.blks) {
            // HAB (hat.py:220-271): x = x + proj(attn(u)) + conv_scale * CAB(u), u = norm1(x); then the MLP
            HT(ln(s, X, O, PP(r, k.n1w), PP(r, k.n1b), M, E));
            GemmP p = gp_tok(O, M, E, E, wt + k.qkv.t, 3 * E, PP(r, k.qkv.b), r->A, 3 * E);
            HT(gemm(s, r, p));
            p = gp_conv(O, B, H, W, E, wt + k.c1.t, r->Cc, PP(r, k.c1.b), r->T1, r->Cc);       // CAB (hat.py:36-41)
            p.act = ACT_GELU;
            HT(gemm(s, r, p));
            p = gp_conv(r->T1, B, H, W, r->Cc, wt + k.c2.t, E, PP(r, k.c2.b), r->T2, E);
            HT(gemm(s, r, p));
            HT(pool_partial(s, r->T2, PART, B, HW, E));
            HT(ca(s, PART, B, HW, E, r->Cs, r->params + k.sq1.w, r->params + k.sq1.b, r->params + k.sq2.w, r->params + k.sq2.b, nullptr, r->YC));
            // u is no longer needed: O takes the attention
            HT(attention(s, r->A, O, r->params + k.table, B, H, W, E, L.heads, r->ws, k.shift, attn_scale(c.qk_scale, E / L.heads)));
            p = gp_tok(O, M, E, E, wt + k.proj.t, E, PP(r, k.proj.b), X, E);
            p.res = X; p.rbs = 0; p.rps = E;
            HT(gemm(s, r, p));
            HT(combine(s, X, r->T2, r->YC, (float)c.conv_scale, B, HW, E));
            HT(mlp(s, r, X, O, M, k.n2w, k.n2b, k.fc1, k.fc2));                              // hat.py:269
        }
        {   // OCAB (hat.py:326-396)
            const OBlk& o = L.oca;
            HT(ln(s, X, O, PP(r, o.n1w), PP(r, o.n1b), M, E));
            GemmP p = gp_tok(O, M, E, E, wt + o.qkv.t, 3 * E, PP(r, o.qkv.b), r->A, 3 * E);
            HT(gemm(s, r, p));
            HT(ocab(s, r->A, O, r->params + o.table, B, H, W, E, L.heads, r->ws, r->ow, attn_scale(c.qk_scale, E / L.heads)));
            p = gp_tok(O, M, E, E, wt + o.proj.t, E, PP(r, o.proj.b), X, E);
            p.res = X; p.rbs = 0; p.rps = E;
            HT(gemm(s, r, p));
            HT(mlp(s, r, X, O, M, o.n2w, o.n2b, o.fc1, o.fc2));                              // hat.py:395
        }
        if (c.resi_connection == 0) {
            GemmP p = gp_conv(X, B, H, W, E, wt + L.conv.t, E, PP(r, L.conv.b), O, E);
            p.res = r->R0; p.rbs = HW * E; p.rps = E;
            HT(gemm(s, r, p));
            std::swap(X, O);
        } else {
            HT(combine(s, X, r->R0, nullptr, 1.f, B, HW, E));
        }
    }
    // norm, conv_after_body + conv_first's output, then conv_before_upsample, Upsample, conv_last (hat.py:895, :907-909)
    HT(ln(s, X, O, PP(r, r->norm_w), PP(r, r->norm_b), M, E));
    if (c.resi_connection == 0) {
        GemmP p = gp_conv(O, B, H, W, E, wt + r->after.t, E, PP(r, r->after.b), X, E);
        p.res = XF; p.rbs = HW * E; p.rps = E;
        HT(gemm(s, r, p));
    } else {
        HT(combine(s, O, XF, nullptr, 1.f, B, HW, E));
        std::swap(X, O);
    }
    HT(tail(s, r, X, dev_y, c.in_chans, c.upscale, (float)c.img_range));
#undef HT
    return XSD_OK;
}

// The OCAB's attention on its own (tests): qkv [B][H W][3 C] token rows, table [(ws + ow - 1)^2][heads] -> out [B][H W][C].
int xsd_hat_test_ocab(const float* dev_qkv, const float* dev_table, float* dev_out, int B, int H, int W, int C, int heads, int ws, int ow,
                      float scale, void* stream)
{
    if (!dev_qkv || !dev_table || !dev_out) return rfail(XSD_ERR_ARG, "null argument");
    if (B < 1 || H < 1 || W < 1 || ws < 1 || ws > 16 || H % ws || W % ws) return rfail(XSD_ERR_ARG, "HAT OCAB test: bad shape");
    if (heads < 1 || C % heads || C / heads > 32) return rfail(XSD_ERR_ARG, "HAT OCAB test: bad heads");
    if (ow < ws || ow > OC_MAX_OW || (ow - ws) % 2 || ws * (ws + ow) >= (ws + ow - 1) * (ws + ow - 1))
        return rfail(XSD_ERR_ARG, "HAT OCAB test: bad overlap window %d", ow);
    hipError_t e = ocab((hipStream_t)stream, dev_qkv, dev_out, dev_table, B, H, W, C, heads, ws, ow, scale);
    if (e) return rfail(XSD_ERR_HIP, "HAT OCAB test: %s", hipGetErrorString(e));
    return XSD_OK;
}

// The channel attention's global average pool on its own (tests): x [B][HW][C] token-major -> mean [B][C].  Synchronises the stream.
int xsd_hat_test_channel_mean(const float* dev_x, float* dev_mean, int B, int64_t HW, int C, void* stream)
{
    if (!dev_x || !dev_mean) return rfail(XSD_ERR_ARG, "null argument");
    if (B < 1 || B > 65535 || HW < 1 || C < 1 || C > 4096) return rfail(XSD_ERR_ARG, "HAT pool test: bad shape");
    hipStream_t s = (hipStream_t)stream;
    const int nchunk = pool_chunks(HW);
    double* part = nullptr;
    if (xsd::dev_alloc((void**)&part, sizeof(double) * (size_t)B * nchunk * C) != hipSuccess) {
        (void)hipGetLastError();
        return rfail(XSD_ERR_NOMEM, "HAT pool test: allocation failed");
    }
    hipError_t e = pool_partial(s, dev_x, part, B, HW, C);
    if (!e) e = ca(s, part, B, HW, C, 0, nullptr, nullptr, nullptr, nullptr, dev_mean, nullptr);
    hipStreamSynchronize(s);
    xsd::dev_free(part);
    if (e) return rfail(XSD_ERR_HIP, "HAT pool test: %s", hipGetErrorString(e));
    return XSD_OK;
}

// What a HAB does with its CAB branch t, on its own (tests): see include/xsd.h, xsd_hat_test_ca_combine.
int xsd_hat_test_ca_combine(float* dev_x, const float* dev_t, const float* dev_w1, const float* dev_b1, const float* dev_w2, const float* dev_b2,
                            float scale, int B, int64_t HW, int C, int Cs, float* dev_y, void* stream)
{
    if (!dev_x || !dev_t) return rfail(XSD_ERR_ARG, "null argument");
    if (B < 1 || B > 65535) return rfail(XSD_ERR_ARG, "HAT combine test: %d images are outside [1, 65535]", B);
    if (HW < 1 || HW > (1ll << 28)) return rfail(XSD_ERR_ARG, "HAT combine test: %lld pixels are outside [1, 2^28]", (long long)HW);
    if (C < 1 || C > 4096) return rfail(XSD_ERR_ARG, "HAT combine test: %d channels are outside [1, 4096]", C);
    if ((long long)B * HW * C > (1ll << 38)) return rfail(XSD_ERR_ARG, "HAT combine test: %d x %lld x %d elements are too many", B, (long long)HW, C);
    hipStream_t s = (hipStream_t)stream;
    if (!dev_w1) {                                  // the identity branches' x += t * scale
        if (dev_y) return rfail(XSD_ERR_ARG, "HAT combine test: no gates to return without the squeeze weights");
        hipError_t e = combine(s, dev_x, dev_t, nullptr, scale, B, HW, C);
        hipStreamSynchronize(s);
        if (e) return rfail(XSD_ERR_HIP, "HAT combine test: %s", hipGetErrorString(e));
        return XSD_OK;
    }
    if (!dev_b1 || !dev_w2 || !dev_b2) return rfail(XSD_ERR_ARG, "HAT combine test: the squeeze MLP needs both weights and both biases");
    if (Cs < 1 || Cs > 4096) return rfail(XSD_ERR_ARG, "HAT combine test: a squeezed width of %d is outside [1, 4096]", Cs);
    double* part = nullptr;
    float* gates = nullptr;
    if (xsd::dev_alloc((void**)&part, sizeof(double) * (size_t)B * pool_chunks(HW) * C) != hipSuccess ||
        xsd::dev_alloc((void**)&gates, sizeof(float) * (size_t)B * C) != hipSuccess) {
        (void)hipGetLastError();
        if (part) xsd::dev_free(part);
        return rfail(XSD_ERR_NOMEM, "HAT combine test: allocation failed");
    }
    hipError_t e = pool_partial(s, dev_t, part, B, HW, C);
    if (!e) e = ca(s, part, B, HW, C, Cs, dev_w1, dev_b1, dev_w2, dev_b2, nullptr, gates);
    if (!e) e = combine(s, dev_x, dev_t, gates, scale, B, HW, C);
    if (!e && dev_y) e = hipMemcpyAsync(dev_y, gates, sizeof(float) * (size_t)B * C, hipMemcpyDeviceToDevice, s);
    hipStreamSynchronize(s);
    xsd::dev_free(part);
    xsd::dev_free(gates);
    if (e) return rfail(XSD_ERR_HIP, "HAT combine test: %s", hipGetErrorString(e));
    return XSD_OK;
}

} // extern "C"
