// swinir.hip -- the reference's SwinIR (models/transformer/swinir.py:133-395 with the Swin blocks of modules.py), FORWARD ONLY (eval
// mode: DropPath and Dropout are identities), in exact fp32, with all four reconstruction heads: "pixelshuffle" (classical SR),
// "pixelshuffledirect" (lightweight SR), "nearest+conv" (real-world SR) and "" (denoising: x + conv_last(res)), and both
// resi_connection forms ("1conv", "3conv").
//
// The Swin body is SwinFIR's: the GEMM / 3x3 conv, the (shifted-)window attention, the LayerNorm, the weight packing and the per-block
// launch sequence (swin_block) of sw_kernels.h, and the opt-in bf16x6 GEMM of sw_gemm_s3x.h.  What this file adds is what surrounds
// the body:
//   swinir_pad_kernel   check_image_size (swinir.py:328-333): reflect-pads H and W on the right and bottom to multiples of the
//                       constructor's window_size, then (x - mean) * img_range; it touches the in_chans-channel input only.  The
//                       padded, normalised image is conv_first's input and the `x` of the denoising head's x + conv_last(res).
//   the SW_GEMM_EXT addressing of the two GEMM kernels, compiled into this file's instances only: the nearest-2x source of
//                       conv_up1 / conv_up2 (the upsampled image is never made), the NCHW residual of the denoising head, the crop to
//                       [:H upscale, :W upscale] inside conv_last's NCHW store, and UpsampleOneStep's PixelShuffle straight into the
//                       cropped NCHW output.  No pass over a feature map is spent on the pad or the crop.
#define SW_GEMM_EXT 1
#include "sw_kernels.h"
#include "sw_gemm_s3x.h"

namespace {

enum { UP_PIXELSHUFFLE = 0, UP_DIRECT = 1, UP_NEAREST = 2, UP_NONE = 3 };

// y[b][c][py][px] = (x[b][c][reflect(py)][reflect(px)] - mean[c]) * range over the padded Hp x Wp; the pads are < H and < W
__global__ __launch_bounds__(256) void swinir_pad_kernel(const float* x, float* y, int C, int H, int W, int Hp, int Wp, const float* mean,
                                                         float range, long long total)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int px = (int)(i % Wp);
    const long long t = i / Wp;
    const int py = (int)(t % Hp);
    const long long bc = t / Hp;
    const int c = (int)(bc % C);
    const int sy = py < H ? py : 2 * (H - 1) - py, sx = px < W ? px : 2 * (W - 1) - px;      // F.pad(..., "reflect"): the edge is not repeated
    const float v = x[(bc * H + sy) * W + sx];
    y[i] = (v - (mean ? mean[c] : 0.f)) * range;
}

hipError_t pad(hipStream_t s, const float* x, float* y, int B, int C, int H, int W, int Hp, int Wp, const float* mean, float range)
{
    const long long total = (long long)B * C * Hp * Wp;
    hipLaunchKernelGGL(swinir_pad_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, y, C, H, W, Hp, Wp, mean, range, total);
    return hipGetLastError();
}

int pad_of(int n, int ws) { return (ws - n % ws) % ws; }

struct RLayer {
    std::vector<SBlk> blks;
    int heads;
    Lin c0, c1, c2;              // 1conv: conv (c0); 3conv: conv.0, conv.2, conv.4
};

} // namespace

struct xsd_swinir : SwBase {
    xsd_swinir_config cfg;
    bool clamped = false;
    int E4 = 0;                       // 3conv: embed_dim / 4
    int inH = 0, inW = 0;             // the input size the workspace is planned for (H and W of SwBase are the padded ones)
    std::vector<RLayer> layers;
    Lin after1, after2;               // 3conv: conv_after_body.2 / .4 (SwBase::after is .0)
    Lin up1, up2, hr;                 // nearest+conv
    float* PX = nullptr;              // the padded, normalised input [B][in_chans][Hp][Wp]
};

namespace {

// the three forms of the conv behind an RSTB's blocks and of conv_after_body, in registration order
void resi(xsd_swinir* r, long long& off, Lin& c0, Lin& c1, Lin& c2)
{
    const int E = r->E;
    if (r->cfg.resi_connection == 0) {
        lin(c0, off, E, E, 9, true);
    } else {
        lin(c0, off, r->E4, E, 9, true);
        lin(c1, off, r->E4, r->E4, 1, true);
        lin(c2, off, E, r->E4, 9, true);
    }
}

// the reference's registration order (swinir.py:201-316; modules.py BasicLayer / SwinTransformerBlock / WindowAttention / Mlp)
void layout(xsd_swinir* r)
{
    const auto& c = r->cfg;
    const int E = r->E, side = 2 * r->ws - 1, nf = r->nfeat;
    long long off = 0;
    lin(r->first_l, off, E, c.in_chans, 9, true);
    if (c.patch_norm) { r->pen_w = add(off, E); r->pen_b = add(off, E); }
    for (int li = 0; li < c.num_layers; ++li) {
        RLayer L;
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
        resi(r, off, L.c0, L.c1, L.c2);
        r->layers.push_back(L);
    }
    r->norm_w = add(off, E); r->norm_b = add(off, E);
    resi(r, off, r->after, r->after1, r->after2);
    const int up = c.upscale;
    if (c.upsampler == UP_PIXELSHUFFLE) {
        lin(r->before, off, nf, E, 9, true);
        const int f = up_factor(up);
        for (int s = 0; s < up_stages(up); ++s) {
            Lin u;
            lin(u, off, f * f * nf, nf, 9, true);
            r->ups.push_back(u);
        }
        lin(r->last, off, c.in_chans, nf, 9, true);
    } else if (c.upsampler == UP_DIRECT) {
        Lin u;
        lin(u, off, up * up * c.in_chans, E, 9, true);                         // UpsampleOneStep (modules.py:398-415)
        r->ups.push_back(u);
    } else if (c.upsampler == UP_NEAREST) {
        lin(r->before, off, nf, E, 9, true);
        lin(r->up1, off, nf, nf, 9, true);
        if (up == 4) lin(r->up2, off, nf, nf, 9, true);
        lin(r->hr, off, nf, nf, 9, true);
        lin(r->last, off, c.in_chans, nf, 9, true);
    } else {
        lin(r->last, off, c.in_chans, E, 9, true);
    }
    r->nparams = off;
    r->lins.push_back(&r->first_l);
    for (auto& L : r->layers) {
        for (auto& k : L.blks)
            for (Lin* p : {&k.qkv, &k.proj, &k.fc1, &k.fc2}) r->lins.push_back(p);
        for (Lin* p : {&L.c0, &L.c1, &L.c2})
            if (p->cout) r->lins.push_back(p);
    }
    for (Lin* p : {&r->after, &r->after1, &r->after2, &r->before})
        if (p->cout) r->lins.push_back(p);
    for (auto& u : r->ups) r->lins.push_back(&u);
    for (Lin* p : {&r->up1, &r->up2, &r->hr, &r->last})
        if (p->cout) r->lins.push_back(p);
    long long t = 0;
    for (Lin* p : r->lins) p->t = add(t, (long long)p->cout * p->cin * p->taps);
    r->wt_floats = t;
}

// the factor by which the head enlarges the padded image: "" leaves it as it is whatever upscale says
int head_factor(const xsd_swinir_config& c) { return c.upsampler == UP_NONE ? 1 : c.upscale; }

// workspace of B padded images of Hp x Wp in floats; with `assign` set, also the pointers into r->ws_buf
long long plan_ws(xsd_swinir* r, int B, int Hp, int Wp, bool assign)
{
    const auto& c = r->cfg;
    const long long M = (long long)B * Hp * Wp, E = r->E;
    const bool feat = c.upsampler == UP_PIXELSHUFFLE || c.upsampler == UP_NEAREST;
    const long long up = feat ? (long long)c.upscale * c.upscale : 0;
    const long long sizes[9] = {M * E, M * E, M * std::max({3 * E, (long long)r->hid, 2 * E}), M * E, M * E, M * c.in_chans,
                                feat ? M * r->nfeat : 0, M * up * r->nfeat, M * up * r->nfeat};
    float** ptrs[9] = {&r->XF, &r->X, &r->A, &r->O, &r->R0, &r->PX, &r->V, &r->U0, &r->U1};
    long long off = 0;
    for (int i = 0; i < 9; ++i) {
        if (assign) *ptrs[i] = (float*)r->ws_buf + off;
        off += (std::max(sizes[i], 1ll) + 63) / 64 * 64;        // 256-B aligned
    }
    return off;
}

// conv (1conv) or conv.0 -> LeakyReLU(0.2) -> conv.2 (1x1) -> LeakyReLU(0.2) -> conv.4 (3conv) from `in` into `out`, + res (token-major)
hipError_t resi_conv(hipStream_t s, const xsd_swinir* r, const Lin& c0, const Lin& c1, const Lin& c2, const float* in, float* out,
                     const float* res, int B, int H, int W)
{
    const int E = r->E, E4 = r->E4;
    const long long HW = (long long)H * W, M = B * HW;
    const float* wt = r->wt;
    hipError_t e;
    if (r->cfg.resi_connection != 0) {
        float* T1 = r->A;
        float* T2 = r->A + M * E4;
        GemmP p = gp_conv(in, B, H, W, E, wt + c0.t, E4, PP(r, c0.b), T1, E4);
        p.act = ACT_LRELU; p.slope = 0.2f;
        if ((e = gemm(s, r, p))) return e;
        p = gp_tok(T1, M, E4, E4, wt + c1.t, E4, PP(r, c1.b), T2, E4);
        p.act = ACT_LRELU; p.slope = 0.2f;
        if ((e = gemm(s, r, p))) return e;
        p = gp_conv(T2, B, H, W, E4, wt + c2.t, E, PP(r, c2.b), out, E);
        p.res = res; p.rbs = HW * E; p.rps = E;
        return gemm(s, r, p);
    }
    GemmP p = gp_conv(in, B, H, W, E, wt + c0.t, E, PP(r, c0.b), out, E);
    p.res = res; p.rbs = HW * E; p.rps = E;
    return gemm(s, r, p);
}

// the NCHW store of the network's output: x / img_range + mean, cropped to Ho x Wo where that is less than the h x w the conv covers
void out_nchw(GemmP& p, const xsd_swinir* r, int h, int w, int Ho, int Wo)
{
    const int C = r->cfg.in_chans;
    p.omode = O_NCHW; p.omean = r->mean; p.orange = (float)r->cfg.img_range;
    p.ybs = (long long)C * h * w;
    if (Ho != h || Wo != w) { p.cH = Ho; p.cW = Wo; p.ybs = (long long)C * Ho * Wo; }
}

const char* resi_name(int u) { return u == 0 ? "1conv" : (u == 1 ? "3conv" : "(unknown)"); }

int out_size(const xsd_swinir* r, int H, int W, int* Ho, int* Wo, int* Hp, int* Wp)
{
    const auto& c = r->cfg;
    if (H < 1 || W < 1) return rfail(XSD_ERR_ARG, "SwinIR: bad image size %d x %d", H, W);
    const int ph = pad_of(H, c.window_size), pw = pad_of(W, c.window_size);
    if (ph >= H || pw >= W)
        return rfail(XSD_ERR_ARG, "SwinIR: the reflect pad to a multiple of window_size %d (%d rows, %d columns) must be smaller than the image "
                     "(H = %d, W = %d), as in F.pad", c.window_size, ph, pw, H, W);
    *Hp = H + ph; *Wp = W + pw;
    if (*Hp % r->ws || *Wp % r->ws)
        return rfail(XSD_ERR_ARG, "SwinIR: the padded size %d x %d (multiples of window_size %d) is no multiple of the effective window %d, "
                     "which img_size // patch_size clamped (window_partition)", *Hp, *Wp, c.window_size, r->ws);
    const long long f = head_factor(c);
    if ((long long)*Hp * *Wp * f * f > (1ll << 28)) return rfail(XSD_ERR_ARG, "SwinIR: image of %d x %d pixels is too large", H, W);
    *Ho = (int)std::min<long long>((long long)H * c.upscale, *Hp * f);          // x[:, :, :H * upscale, :W * upscale] of what the head made
    *Wo = (int)std::min<long long>((long long)W * c.upscale, *Wp * f);
    return XSD_OK;
}

} // namespace

extern "C" {

int xsd_swinir_create(const xsd_swinir_config* cfg, xsd_swinir** out)
{
    if (!cfg || !out) return rfail(XSD_ERR_ARG, "null argument");
    const auto& c = *cfg;
    if (c.ape) return rfail(XSD_ERR_ARG, "SwinIR: ape=True (absolute position embedding) is not supported by the MI355X engine");
    if (c.upsampler < 0 || c.upsampler > 3) return rfail(XSD_ERR_ARG, "SwinIR: unknown upsampler %d", c.upsampler);
    if (c.resi_connection != 0 && c.resi_connection != 1)
        return rfail(XSD_ERR_ARG, "SwinIR: resi_connection %s is not supported (\"1conv\" or \"3conv\")", resi_name(c.resi_connection));
    if (int rc = check_dims(c, "SwinIR", true)) return rc;
    if (c.upsampler == UP_NEAREST && c.upscale != 2 && c.upscale != 4)
        return rfail(XSD_ERR_ARG, "SwinIR: upsampler \"nearest+conv\" takes upscale 2 or 4 (got upscale %d: the reference's output size would "
                     "disagree with it)", c.upscale);
    const int res = std::min(c.img_size[0] / c.patch_size[0], c.img_size[1] / c.patch_size[1]);
    const bool clamped = res <= c.window_size;                      // SwinTransformerBlock.__init__ (modules.py:236-239): no shift then
    const int ws = clamped ? res : c.window_size;
    if (ws < 1) return rfail(XSD_ERR_ARG, "SwinIR: img_size // patch_size is 0");
    if (ws > 16) return rfail(XSD_ERR_ARG, "SwinIR: an effective window of %d exceeds the engine's 16 (256 tokens per window)", ws);
    if (int rc = check_layers(c, "SwinIR")) return rc;
    if (c.resi_connection == 1 && c.embed_dim < 4) return rfail(XSD_ERR_ARG, "SwinIR: resi_connection \"3conv\" needs embed_dim >= 4 (got %d)", c.embed_dim);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return rfail(XSD_ERR_HIP, "no HIP device available");
    xsd_swinir* r = new xsd_swinir();
    r->cfg = c;
    r->E = c.embed_dim;
    r->E4 = c.embed_dim / 4;
    r->hid = (int)(c.embed_dim * c.mlp_ratio);
    r->ws = ws;
    r->clamped = clamped;
    layout(r);
    std::vector<float> mean(c.in_chans, 0.f);
    if (c.in_chans == 3) { mean[0] = 0.4488f; mean[1] = 0.4371f; mean[2] = 0.4040f; }   // swinir.py:190-194
    if (int rc = alloc_weights(r, "SwinIR", mean)) {
        delete r;
        return rc;
    }
    *out = r;
    return XSD_OK;
}

void xsd_swinir_destroy(xsd_swinir* r) { delete r; }

int64_t xsd_swinir_param_count(const xsd_swinir* r) { return r ? r->nparams : -1; }

int xsd_swinir_pack_weights(xsd_swinir* r, const float* dev_params, void* stream)
{
    return pack_weights(r, "SwinIR", dev_params, stream);
}

int xsd_swinir_set_math(xsd_swinir* r, int mode) { return set_math(r, "SwinIR", mode); }

int xsd_swinir_get_math(const xsd_swinir* r) { return r ? r->math : -1; }

int xsd_swinir_out_size(const xsd_swinir* r, int H, int W, int* Ho, int* Wo)
{
    if (!r || !Ho || !Wo) return rfail(XSD_ERR_ARG, "null argument");
    int Hp = 0, Wp = 0;
    return out_size(r, H, W, Ho, Wo, &Hp, &Wp);
}

int xsd_swinir_forward(xsd_swinir* r, const float* dev_x, float* dev_y, int B, int H, int W, void* stream)
{
    if (!r || !dev_x || !dev_y) return rfail(XSD_ERR_ARG, "null argument");
    if (B < 1 || H < 1 || W < 1) return rfail(XSD_ERR_ARG, "bad shape %dx%dx%d", B, H, W);
    int Ho = 0, Wo = 0, Hp = 0, Wp = 0;
    if (int rc = out_size(r, H, W, &Ho, &Wo, &Hp, &Wp)) return rc;
    if (!r->packed) return rfail(XSD_ERR_STATE, "xsd_swinir_pack_weights must be called before xsd_swinir_forward");
    if (int rc = ready_math(r, "SwinIR", (hipStream_t)stream)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (r->B != B || r->inH != H || r->inW != W) {
        int rc = grow_ws(r, "SwinIR", plan_ws(r, B, Hp, Wp, false), B, Hp, Wp);
        if (rc) return rc;
        plan_ws(r, B, Hp, Wp, true);
        r->B = B; r->H = Hp; r->W = Wp; r->inH = H; r->inW = W;
    }
    const auto& c = r->cfg;
    const int E = r->E, C = c.in_chans, nf = r->nfeat;
    const long long HW = (long long)Hp * Wp, M = B * HW;
    float* X = r->X;
    float* O = r->O;
    float* const XF = r->XF;
    const float* wt = r->wt;
    const float range = (float)c.img_range;
    hipError_t e = hipSuccess;
#define SW(x) do { if ((e = (x)) != hipSuccess) return rfail(XSD_ERR_HIP, "SwinIR forward: %s (%s:%d)", hipGetErrorString(e), __FILE__, __LINE__); } while (0)
    // check_image_size, then (x - mean) * img_range (swinir.py:351-355); conv_first; patch_embed (modules.py:455-461)
    SW(pad(s, dev_x, r->PX, B, C, H, W, Hp, Wp, r->mean, range));
    {
        GemmP p = gp_conv(r->PX, B, Hp, Wp, C, wt + r->first_l.t, E, PP(r, r->first_l.b), XF, E);
        p.acs = HW; p.aps = 1;
        SW(gemm(s, r, p));
    }
    if (c.patch_norm) SW(ln(s, XF, X, PP(r, r->pen_w), PP(r, r->pen_b), M, E));
    else SW(hipMemcpyAsync(X, XF, sizeof(float) * M * E, hipMemcpyDeviceToDevice, s));
    for (const RLayer& L : r->layers) {
        // the RSTB's input: its `+ x` (swinir.py:114-120) adds it after the blocks and the conv
        SW(hipMemcpyAsync(r->R0, X, sizeof(float) * M * E, hipMemcpyDeviceToDevice, s));
        for (const SBlk& k : L.blks) SW(swin_block(s, r, k, X, O, B, Hp, Wp, L.heads, attn_scale(c.qk_scale, E / L.heads)));
        SW(resi_conv(s, r, L.c0, L.c1, L.c2, X, O, r->R0, B, Hp, Wp));
        std::swap(X, O);
    }
    // norm, conv_after_body + conv_first's output (swinir.py:345, :360 / :366 / :371 / :390)
    SW(ln(s, X, O, PP(r, r->norm_w), PP(r, r->norm_b), M, E));
    SW(resi_conv(s, r, r->after, r->after1, r->after2, O, X, XF, B, Hp, Wp));
    if (c.upsampler == UP_PIXELSHUFFLE) {
        // conv_before_upsample, Upsample, conv_last (swinir.py:361-362), cropped in conv_last's store
        const bool crop = Ho != Hp * c.upscale || Wo != Wp * c.upscale;
        SW(tail(s, r, X, dev_y, C, c.upscale, range, crop ? Ho : 0, crop ? Wo : 0));
    } else if (c.upsampler == UP_DIRECT) {
        // UpsampleOneStep (swinir.py:367): one conv, its PixelShuffle, the output affine and the crop in the store
        GemmP p = gp_conv(X, B, Hp, Wp, E, wt + r->ups[0].t, c.upscale * c.upscale * C, PP(r, r->ups[0].b), dev_y, 0);
        p.omode = O_SHUFFLE_NCHW; p.r = c.upscale; p.cH = Ho; p.cW = Wo; p.ybs = (long long)C * Ho * Wo;
        p.omean = r->mean; p.orange = range;
        SW(gemm(s, r, p));
    } else if (c.upsampler == UP_NEAREST) {
        // swinir.py:372-386; the nearest-2x images are read through the conv's addressing, never stored
        GemmP p = gp_conv(X, B, Hp, Wp, E, wt + r->before.t, nf, PP(r, r->before.b), r->V, nf);
        p.act = ACT_LRELU; p.slope = 0.01f;
        SW(gemm(s, r, p));
        p = gp_conv_up2(r->V, B, Hp, Wp, nf, wt + r->up1.t, nf, PP(r, r->up1.b), r->U0, nf);
        p.act = ACT_LRELU; p.slope = 0.2f;
        SW(gemm(s, r, p));
        float* cur = r->U0;
        float* oth = r->U1;
        int h = 2 * Hp, w = 2 * Wp;
        if (c.upscale == 4) {
            p = gp_conv_up2(cur, B, h, w, nf, wt + r->up2.t, nf, PP(r, r->up2.b), oth, nf);
            p.act = ACT_LRELU; p.slope = 0.2f;
            SW(gemm(s, r, p));
            std::swap(cur, oth);
            h *= 2; w *= 2;
        }
        p = gp_conv(cur, B, h, w, nf, wt + r->hr.t, nf, PP(r, r->hr.b), oth, nf);
        p.act = ACT_LRELU; p.slope = 0.2f;
        SW(gemm(s, r, p));
        p = gp_conv(oth, B, h, w, nf, wt + r->last.t, C, PP(r, r->last.b), dev_y, 0);
        out_nchw(p, r, h, w, Ho, Wo);
        SW(gemm(s, r, p));
    } else {
        // x + conv_last(res) on the padded, normalised image (swinir.py:389-391)
        GemmP p = gp_conv(X, B, Hp, Wp, E, wt + r->last.t, C, PP(r, r->last.b), dev_y, 0);
        p.res = r->PX; p.rbs = (long long)C * HW; p.rnchw = 1;
        out_nchw(p, r, Hp, Wp, Ho, Wo);
        SW(gemm(s, r, p));
    }
#undef SW
    return XSD_OK;
}

// Step 1 of the forward on its own (tests): see include/xsd.h, xsd_swinir_test_pad.
int xsd_swinir_test_pad(const float* dev_x, float* dev_y, int B, int C, int H, int W, int ws, const float* mean, float img_range, void* stream)
{
    if (!dev_x || !dev_y) return rfail(XSD_ERR_ARG, "null argument");
    if (B < 1 || C < 1 || C > 64 || H < 1 || W < 1 || ws < 1) return rfail(XSD_ERR_ARG, "SwinIR pad test: bad shape");
    const int ph = pad_of(H, ws), pw = pad_of(W, ws);
    if (ph >= H || pw >= W)
        return rfail(XSD_ERR_ARG, "SwinIR pad test: the reflect pad (%d rows, %d columns) must be smaller than the image (H = %d, W = %d)", ph, pw, H, W);
    if ((long long)B * C * (H + ph) * (W + pw) > (1ll << 31)) return rfail(XSD_ERR_ARG, "SwinIR pad test: too many elements");
    hipStream_t s = (hipStream_t)stream;
    float* dmean = nullptr;
    if (mean) {
        if (xsd::dev_alloc((void**)&dmean, sizeof(float) * C) != hipSuccess) {
            (void)hipGetLastError();
            return rfail(XSD_ERR_NOMEM, "SwinIR pad test: allocation failed");
        }
        if (hipMemcpy(dmean, mean, sizeof(float) * C, hipMemcpyHostToDevice) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {      // on the device before the kernel on `s` reads it
            xsd::dev_free(dmean);
            return rfail(XSD_ERR_HIP, "SwinIR pad test: upload of the mean failed");
        }
    }
    hipError_t e = pad(s, dev_x, dev_y, B, C, H, W, H + ph, W + pw, dmean, img_range);
    hipStreamSynchronize(s);
    if (dmean) xsd::dev_free(dmean);
    if (e) return rfail(XSD_ERR_HIP, "SwinIR pad test: %s", hipGetErrorString(e));
    return XSD_OK;
}

// conv_up1 / conv_up2 with their activation on their own (tests): see include/xsd.h, xsd_swinir_test_nearest_conv.
int xsd_swinir_test_nearest_conv(const float* dev_a, const float* dev_w, const float* dev_bias, float* dev_y, int B, int H, int W, int cin, int N,
                                 float slope, int math, void* stream)
{
    return test_gemm(dev_a, dev_w, dev_bias, dev_y, 1, B, H, W, cin, N, N, ACT_LRELU, slope, math, (hipStream_t)stream, true);
}

// One launch of the SW_GEMM_EXT instances as the forward describes its own (tests): see include/xsd.h, xsd_swinir_test_gemm_view.
int xsd_swinir_test_gemm_view(const xsd_sw_gemm_view* view, void* stream) { return test_gemm_view(view, (hipStream_t)stream); }

} // extern "C"
