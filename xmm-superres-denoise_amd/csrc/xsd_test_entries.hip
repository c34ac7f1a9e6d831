// xsd_test_entries.hip -- the kernel-level test entries of the C ABI (include/xsd.h: xsd_test_*, xsd_loss_test_*): one launch, one
// packer or one buffer of the engine at a time, for the tests that pin the kernels one by one.  Host code only, no kernel lives here.
//
// The rule: an entry never writes an engine sequence out again, it calls the function the engine calls -- the view arithmetic
// (PlaneViews), the panel packer (pack_panels), the launchers and the part-count rules of xsd_engine_impl.h -- so a change to the
// engine reaches the tests with it.  The file reads nothing from the environment and depends on no build variant: the same object
// is linked into the product and into the hooks library.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "xsd_loss.h"
#include "xsd_engine_impl.h"

// The one tail of a synchronous entry: wait for the stream whatever happened, then a HIP error is the entry's failure "<what>: <error>".
static int finish(hipError_t err, hipStream_t s, const char* what)
{
    const hipError_t serr = hipStreamSynchronize(s);
    if (err == hipSuccess) err = serr;
    if (err != hipSuccess) return fail(XSD_ERR_HIP, "%s: %s", what, hipGetErrorString(err));
    return XSD_OK;
}

// The device allocations of one entry call: freed when the call returns, whichever way it returns.
namespace {
struct DevMem {
    std::vector<void*> ptrs;
    template <class T> hipError_t alloc(T** p, size_t n)
    {
        const hipError_t err = xsd::dev_alloc((void**)p, sizeof(T) * n);
        if (err == hipSuccess) ptrs.push_back(*p);
        return err;
    }
    ~DevMem() { for (void* p : ptrs) xsd::dev_free(p); }
};
} // namespace

// Math mode 4, nobody has reported these planes' max |x|: zero their borrowed slots, sweep each plane into its slot, hand the slots to the launch.
static hipError_t reduce_amax(const PlaneIn* planes, int n, float* slots, const float** launch_slots, int B, int H, int W, hipStream_t s)
{
    hipError_t err = hipMemsetAsync(slots, 0, 5 * sizeof(float), s);
    for (int i = 0; i < n && err == hipSuccess; ++i) { err = launch_plane_amax(planes[i], B, H, W, slots + i, s); launch_slots[i] = slots + i; }
    return err;
}

extern "C" {

// ---- single-layer test entries ---------------------------------------------------------------------------------
// one conv's OIHW weights through pack_panels, as xsd_pack_weights packs the net's: *fwd / *bwd are the panels the engine's math mode
// reads; mode 4 leaves max |w| in the borrowed slots w_fwd / w_bwd.  Everything is stream-ordered and belongs to `mem`.
static int pack_single(xsd_engine* e, const float* dev_w, int cout, int cin, DevMem& mem, float** fwd, float** bwd, hipStream_t s)
{
    const long long n = (long long)(cout / 32) * (cin / 32) * PANEL_FLOATS;
    PackDesc d; d.src_w = 0; d.dst_fwd = 0; d.dst_bwd = 0; d.cout = cout; d.cin = cin; d.shuffle = 0; d.bwd_scale = 1.f;
    PackDesc* dd = nullptr;
    float *tf = nullptr, *tb = nullptr;      // mode 4: the fp32 panels the two-term fp16 images are split from
    HIPCHK(mem.alloc(fwd, n));
    HIPCHK(mem.alloc(bwd, n));
    HIPCHK(mem.alloc(&dd, 1));
    HIPCHK(hipMemcpy(dd, &d, sizeof(d), hipMemcpyHostToDevice));
    if (e->math == 4) { HIPCHK(mem.alloc(&tf, n)); HIPCHK(mem.alloc(&tb, n)); }
    HIPCHK(pack_panels(e->math, dev_w, dd, 1, e->math == 4 ? tf : *fwd, e->math == 4 ? tb : *bwd, *fwd, *bwd, n, test_slots(e).w_fwd, s));
    return XSD_OK;
}

static xsd_test_out plain_out(float* p, float slope)      // an output chunk with no epilogue but a LeakyReLU slope (1: none)
{
    xsd_test_out t; memset(&t, 0, sizeof(t));
    t.p = p; t.a1 = 1.f; t.a2 = 1.f; t.slope = slope; t.mslope = 1.f;
    return t;
}

// One conv launch over packed panels, every conv entry's: planes and views from PlaneViews, the launch through launch_conv_any.
// report_out: in mode 4 the output chunks report their max |x| into the borrowed slots `out` (else OutDesc::amax stays null).
static hipError_t conv_single(xsd_engine* e, const PlaneViews& v, const float* const* in_planes, int n_in, int shuffle_in, const float* wpanel,
                              const float* amax_w, const float* bias, const xsd_test_out* outs, int n_out, int shuffle_out, bool report_out, hipStream_t s)
{
    const TestSlots slots = test_slots(e);
    report_out = report_out && e->math == 4;
    ConvParams p = v.conv_base(0);
    p.n_in = n_in; p.n_out = n_out; p.wpanel = wpanel; p.bias = bias;
    p.amax_w = amax_w;                         // mode 4: max |w| of these panels (pack_single)
    for (int i = 0; i < n_in; ++i) p.in[i] = shuffle_in ? v.shuf_in(in_planes[0], 0, i) : v.std_in(in_planes[i], 0);
    for (int j = 0; j < n_out; ++j) {
        const xsd_test_out& t = outs[j];
        OutDesc& o = p.out[j];
        if (shuffle_out) v.shuf_out(o, outs[0].p, 0, j); else v.std_out(o, t.p, 0);
        o.e1 = t.e1; o.e2 = t.e2; o.e3 = t.e3; o.mask = t.mask;
        o.a1 = t.a1; o.s1 = t.s1; o.a2 = t.a2; o.s2 = t.s2; o.s3 = t.s3; o.slope = t.slope; o.mslope = t.mslope;
        o.accumulate = t.accumulate; o.bits_out = t.bits_out; o.bits_in = t.bits_in;
        if (report_out) o.amax = slots.out + j;
    }
    p.zero = e->zero_page;
    p.ablate = e->ablate;      // (0 outside the diagnostic library)
    for (int i = 0; i < (n_out > 1 ? n_out : n_in); ++i) p.wstep[i] = p.wpanel + (long long)i * PANEL_FLOATS;
    hipError_t err = report_out ? hipMemsetAsync(slots.out, 0, 5 * sizeof(float), s) : hipSuccess;
    if (err == hipSuccess && e->math == 4) err = reduce_amax(p.in, n_in, slots.in, p.amax_in, p.B, p.H, p.W, s);
    if (err == hipSuccess) err = launch_conv_any(e, p, s);
    return err;
}

// One weight-gradient launch over the n_in x n_g rectangle plus its fixed-order reduction, every single-launch weight-gradient entry's.
// `rp` arrives with the caller's fields (the conv's extent, the launch's place in it, scale, dw, db); the launch's own are filled here.
static hipError_t wgrad_single(xsd_engine* e, const PlaneViews& v, const float* const* x_planes, int n_in, const float* const* g_planes, int n_g,
                               int shuffle_g, int nparts, WgradReduceParams rp, hipStream_t s)
{
    const TestSlots slots = test_slots(e);
    WgradParams wp = v.wgrad_base(0);
    wp.n_in = n_in; wp.n_g = n_g; wp.nparts = nparts;
    for (int i = 0; i < n_in; ++i) wp.x[i] = v.std_in(x_planes[i], 0);
    for (int i = 0; i < n_g; ++i) wp.g[i] = shuffle_g ? v.shuf_in(g_planes[0], 0, i) : v.std_in(g_planes[i], 0);
    wp.partial = e->wg_partial; wp.bias_partial = e->wg_bias_partial; wp.zero = e->zero_page; wp.ablate = e->ablate;
    hipError_t err = hipSuccess;
    if (e->math == 4) {
        err = reduce_amax(wp.x, n_in, slots.x, wp.amax_x, wp.B, wp.H, wp.W, s);
        if (err == hipSuccess) err = reduce_amax(wp.g, n_g, slots.g, wp.amax_g, wp.B, wp.H, wp.W, s);
    }
    if (err == hipSuccess) err = e->math >= 3 ? launch_wgrad_split(e->math, e->ablate, wp, s) : launch_wgrad_mfma(wp, s);
    if (err == hipSuccess) {
        rp.partial = e->wg_partial; rp.bias_partial = e->wg_bias_partial; rp.nparts = nparts; rp.n_in = n_in; rp.n_g = n_g;
        err = launch_wgrad_reduce(rp, s);
    }
    return err;
}

int xsd_test_conv3x3(xsd_engine* e, const float* const* in_planes, int n_in, const float* dev_w_oihw, const float* dev_bias,
                     float* const* out_planes, int n_out, float slope, int B, int H, int W, void* stream)
{
    if (!e || n_in < 1 || n_in > 5 || n_out < 1 || n_out > 5 || (n_in > 1 && n_out > 1)) return fail(XSD_ERR_ARG, "bad n_in/n_out");
    if (e->generic) return fail(XSD_ERR_ARG, "single-layer test hooks exist for the 32-filter MFMA path only");
    hipStream_t s = (hipStream_t)stream;
    DevMem mem;
    float *fwd = nullptr, *bwd = nullptr;
    int rc = pack_single(e, dev_w_oihw, 32 * n_out, 32 * n_in, mem, &fwd, &bwd, s);
    if (rc) return rc;
    xsd_test_out outs[5];
    for (int j = 0; j < n_out; ++j) outs[j] = plain_out(out_planes[j], slope);
    return finish(conv_single(e, PlaneViews{B, H, W}, in_planes, n_in, 0, fwd, test_slots(e).w_fwd, dev_bias, outs, n_out, 0, false, s), s, "conv launch");
}

int xsd_test_conv3x3_bwd(xsd_engine* e, const float* const* in_planes, int n_in, const float* dev_w_oihw, const float* dev_g_plane,
                         float* const* dx_planes, float* dev_dw_oihw, float* dev_db, int B, int H, int W, void* stream)
{
    if (!e || n_in < 1 || n_in > 5) return fail(XSD_ERR_ARG, "bad n_in");
    if (e->generic) return fail(XSD_ERR_ARG, "single-layer test hooks exist for the 32-filter MFMA path only");
    hipStream_t s = (hipStream_t)stream;
    DevMem mem;
    float *fwd = nullptr, *bwd = nullptr;
    int rc = pack_single(e, dev_w_oihw, 32, 32 * n_in, mem, &fwd, &bwd, s);
    if (rc) return rc;
    const PlaneViews v{B, H, W};
    xsd_test_out outs[5];
    for (int j = 0; j < n_in; ++j) outs[j] = plain_out(dx_planes[j], 1.f);
    // the input gradient: one G plane through the transposed panels into n_in chunks; then the weight gradient over all of the batch's parts
    hipError_t err = conv_single(e, v, &dev_g_plane, 1, 0, bwd, test_slots(e).w_bwd, nullptr, outs, n_in, 0, false, s);
    if (err == hipSuccess) {
        WgradReduceParams rp; memset(&rp, 0, sizeof(rp));
        rp.cin_total = 32 * n_in; rp.cout_total = 32; rp.shuffle = 0; rp.scale = 1.f; rp.dw = dev_dw_oihw; rp.db = dev_db;
        err = wgrad_single(e, v, in_planes, n_in, &dev_g_plane, 1, 0, e->nparts, rp, s);
    }
    return finish(err, s, "bwd launch");
}

// One conv launch with a caller-supplied epilogue per output chunk and, optionally, pixel-shuffled views on either side (include/xsd.h).
int xsd_test_conv3x3_ex(xsd_engine* e, const float* const* in_planes, int n_in, int shuffle_in, const float* dev_w_oihw, const float* dev_bias,
                        const xsd_test_out* outs, int n_out, int shuffle_out, float* host_amax11, int B, int H, int W, void* stream)
{
    if (!e || !in_planes || !outs || !dev_w_oihw || B < 1 || H < 1 || W < 1) return fail(XSD_ERR_ARG, "null argument or empty shape");
    if (n_in < 1 || n_in > 5 || n_out < 1 || n_out > 5 || (n_in > 1 && n_out > 1)) return fail(XSD_ERR_ARG, "bad n_in/n_out");
    if ((shuffle_in && n_in != 4) || (shuffle_out && n_out != 4)) return fail(XSD_ERR_ARG, "a pixel-shuffled side has exactly four views");
    if (e->generic) return fail(XSD_ERR_ARG, "single-layer test hooks exist for the 32-filter MFMA path only");
    for (int i = 0; i < (shuffle_in ? 1 : n_in); ++i) if (!in_planes[i]) return fail(XSD_ERR_ARG, "null input plane");
    for (int j = 0; j < (shuffle_out ? 1 : n_out); ++j) if (!outs[j].p) return fail(XSD_ERR_ARG, "null output plane");
    hipStream_t s = (hipStream_t)stream;
    DevMem mem;
    float *fwd = nullptr, *bwd = nullptr;
    int rc = pack_single(e, dev_w_oihw, 32 * n_out, 32 * n_in, mem, &fwd, &bwd, s);
    if (rc) return rc;
    const TestSlots slots = test_slots(e);
    rc = finish(conv_single(e, PlaneViews{B, H, W}, in_planes, n_in, shuffle_in, fwd, slots.w_fwd, dev_bias, outs, n_out, shuffle_out, true, s), s, "conv launch");
    if (rc || !host_amax11) return rc;
    for (int k = 0; k < 11; ++k) host_amax11[k] = 0.f;
    if (e->math == 4) {
        hipError_t err = hipMemcpy(host_amax11, slots.in, n_in * sizeof(float), hipMemcpyDeviceToHost);
        if (err == hipSuccess) err = hipMemcpy(host_amax11 + 5, slots.w_fwd, sizeof(float), hipMemcpyDeviceToHost);
        if (err == hipSuccess) err = hipMemcpy(host_amax11 + 6, slots.out, n_out * sizeof(float), hipMemcpyDeviceToHost);
        if (err != hipSuccess) return fail(XSD_ERR_HIP, "conv launch: %s", hipGetErrorString(err));
    }
    return XSD_OK;
}

// One weight-gradient launch over the n_in x n_g rectangle plus its fixed-order reduction, with the reduction's fields from the caller.
int xsd_test_wgrad_ex(xsd_engine* e, const float* const* x_planes, int n_in, const float* const* g_planes, int n_g, int shuffle_g,
                      float scale, int shuffle, int plane, int j0, int n0, int cin_total, int cout_total,
                      float* dev_dw_oihw, float* dev_db, int B, int H, int W, void* stream)
{
    if (!e || !x_planes || !g_planes || !dev_dw_oihw || !dev_db || B < 1 || H < 1 || W < 1) return fail(XSD_ERR_ARG, "null argument or empty shape");
    if (e->generic) return fail(XSD_ERR_ARG, "single-layer test hooks exist for the 32-filter MFMA path only");
    if (n_in < 1 || n_in > 5 || n_g < 1 || n_g > 4) return fail(XSD_ERR_ARG, "bad n_in/n_g (at most 5 X and 4 G planes)");
    if (shuffle_g && n_g != 4) return fail(XSD_ERR_ARG, "a pixel-shuffled G plane has exactly four views");
    if (shuffle && n_g != 4) return fail(XSD_ERR_ARG, "the shuffled reduction takes the four sub-pixel gradients (n_g = 4)");
    const int nparts = wgrad_nparts(e, n_in, n_g);
    // wg_partial holds nparts x 5 panels, wg_bias_partial nparts x 4 x 32 sums (xsd_create)
    if ((long long)nparts * n_in * n_g > (long long)e->nparts * 5) return fail(XSD_ERR_ARG, "%d x %d pairs over %d parts do not fit the partial-sum buffer", n_in, n_g, nparts);
    if (j0 < 0 || n0 < 0 || plane < 0 || cin_total < 32 * (j0 + n_in)) return fail(XSD_ERR_ARG, "the launch's input planes lie outside cin_total");
    if (shuffle ? cout_total < 128 * (plane + 1) : cout_total < 32 * (n0 + n_g)) return fail(XSD_ERR_ARG, "the launch's output chunks lie outside cout_total");
    for (int i = 0; i < n_in; ++i) if (!x_planes[i]) return fail(XSD_ERR_ARG, "null X plane");
    for (int i = 0; i < (shuffle_g ? 1 : n_g); ++i) if (!g_planes[i]) return fail(XSD_ERR_ARG, "null G plane");
    hipStream_t s = (hipStream_t)stream;
    WgradReduceParams rp; memset(&rp, 0, sizeof(rp));
    rp.cin_total = cin_total; rp.cout_total = cout_total; rp.shuffle = shuffle; rp.scale = scale; rp.j0 = j0; rp.n0 = n0; rp.plane = plane;
    rp.dw = dev_dw_oihw; rp.db = dev_db;
    return finish(wgrad_single(e, PlaneViews{B, H, W}, x_planes, n_in, g_planes, n_g, shuffle_g, nparts, rp, s), s, "weight-gradient launch");
}

// A dense block's pair-list weight-gradient launch plus the five convs' reductions (include/xsd.h): the launch and the reductions are
// filled by wgrad_block_fill, the function the plan calls; both partial-sum buffers are all-ones bytes (NaN) when the launch starts.
int xsd_test_wgrad_block(xsd_engine* e, const float* const* x_planes, const float* const* g_planes, float gscale, float* dev_grads,
                         const long long* w_off, const long long* b_off, int nparts, int separate_reduces, int* host_nparts,
                         int B, int H, int W, void* stream)
{
    if (!e || !x_planes || !g_planes || !dev_grads || !w_off || !b_off || B < 1 || H < 1 || W < 1) return fail(XSD_ERR_ARG, "null argument or empty shape");
    if (e->generic) return fail(XSD_ERR_ARG, "single-layer test hooks exist for the 32-filter MFMA path only");
    if (e->math < 3) return fail(XSD_ERR_ARG, "the pair-list launch belongs to the split math modes (bf16x6, f16x3)");
    for (int i = 0; i < 5; ++i) if (!x_planes[i] || !g_planes[i]) return fail(XSD_ERR_ARG, "null X or G plane");
    for (int n = 0; n < 5; ++n) if (w_off[n] < 0 || b_off[n] < 0) return fail(XSD_ERR_ARG, "negative gradient offset");
    if (nparts == 0) nparts = wgrad_block_nparts(e);
    const int m = nparts >> 3;
    if (nparts < 8 || (nparts & 7) > 1 || m > 10) return fail(XSD_ERR_ARG, "nparts = %d: a pair-list launch runs 8 m or 8 m + 1 parts, 1 <= m <= 10", nparts);
    // wg_partial holds e->nparts x 5 panels, wg_bias_partial e->nparts x 4 x 32 sums (xsd_create)
    if ((long long)nparts * 15 > (long long)e->nparts * 5 || (long long)nparts * 5 * 32 > (long long)e->nparts * 4 * 32)
        return fail(XSD_ERR_ARG, "15 panels and 5 x 32 bias sums of %d parts do not fit the partial-sum buffers", nparts);
    hipStream_t s = (hipStream_t)stream;
    const PlaneViews v{B, H, W};
    const TestSlots slots = test_slots(e);
    WgradBlock k;
    k.wp = v.wgrad_base(0);
    for (int i = 0; i < 5; ++i) { k.wp.x[i] = v.std_in(x_planes[i], 0); k.wp.g[i] = v.std_in(g_planes[i], 0); }
    int cin[5], cout[5];
    for (int n = 0; n < 5; ++n) { cin[n] = 32 * (n + 1); cout[n] = 32; }
    wgrad_block_fill(k, nparts, cin, cout, gscale, e->wg_partial, e->wg_bias_partial);
    for (int n = 0; n < 5; ++n) { k.rp[n].dw = dev_grads + w_off[n]; k.rp[n].db = dev_grads + b_off[n]; }
    k.wp.zero = e->zero_page; k.wp.ablate = e->ablate;
    hipError_t err = hipSuccess;
    if (e->math == 4) {
        err = reduce_amax(k.wp.x, 5, slots.x, k.wp.amax_x, B, H, W, s);
        if (err == hipSuccess) err = reduce_amax(k.wp.g, 5, slots.g, k.wp.amax_g, B, H, W, s);
    }
    // a panel or a bias row that no workgroup writes reaches dw / db as NaN, not as the previous launch's value
    if (err == hipSuccess) err = hipMemsetAsync(e->wg_partial, 0xFF, sizeof(float) * (size_t)e->nparts * 5 * PANEL_FLOATS, s);
    if (err == hipSuccess) err = hipMemsetAsync(e->wg_bias_partial, 0xFF, sizeof(float) * (size_t)e->nparts * 4 * 32, s);
    if (err == hipSuccess) err = launch_wgrad_split(e->math, e->ablate, k.wp, s);
    if (err == hipSuccess) err = wgrad_block_reduce(k, separate_reduces != 0, s);
    const int rc = finish(err, s, "weight-gradient block launch");
    if (rc == XSD_OK && host_nparts) *host_nparts = nparts;
    return rc;
}

// ---- the edge layers one by one (include/xsd.h): the engine's packer, the engine's launchers, the engine's block-count rule ----
// one (32, 9) block through pack_edge_kernel; *packed = the form asked for ([tap][c]), in a buffer that belongs to `mem`
static int edge_pack_one(const float* dev_w, int w_last, int flipped, int first_cstride, hipStream_t s, DevMem& mem, const float** packed)
{
    if (!dev_w) return fail(XSD_ERR_ARG, "null weight block");
    if (!w_last && first_cstride < 9) return fail(XSD_ERR_ARG, "first_cstride is 9 * in_channels");
    float* buf = nullptr;
    if (mem.alloc(&buf, 4 * 288) != hipSuccess) return fail(XSD_ERR_NOMEM, "edge weight forms");
    hipError_t err = launch_pack_edge(w_last ? nullptr : dev_w, w_last ? dev_w : nullptr, buf, buf + 288, buf + 576, buf + 864, s, w_last ? 9 : first_cstride);
    if (err != hipSuccess) return fail(XSD_ERR_HIP, "pack_edge launch: %s", hipGetErrorString(err));
    *packed = buf + (w_last ? 576 : 0) + (flipped ? 288 : 0);
    return XSD_OK;
}
static int edge_hook_args(const xsd_engine* e, int B, int H, int W)
{
    if (!e || B < 1 || H < 1 || W < 1) return fail(XSD_ERR_ARG, "null engine or empty shape");
    if (e->generic) return fail(XSD_ERR_ARG, "the edge kernels belong to the plane path");
    if (W > EDGE_MAX_W) return fail(XSD_ERR_ARG, "the edge kernels stage rows of at most %d pixels", EDGE_MAX_W);
    if ((long long)B * H > 0x7fffffffll / W) return fail(XSD_ERR_ARG, "shape too large");
    return XSD_OK;
}

// ---- the generic-width kernels one by one (include/xsd.h): a GenericNet of one conv, its own pack() / conv() / wgrad() / ew() ----
static int gconv_hook_args(int cout, int cin, long long param_off, int B, int H, int W)
{
    if (cout < 1 || cin < 1 || cout > 4096 || cin > 4096 || param_off < 0 || B < 1 || H < 1 || W < 1) return fail(XSD_ERR_ARG, "bad channel counts, offset or shape");
    if ((long long)H * W > (1ll << 24) || (long long)B * H * W > (1ll << 26)) return fail(XSD_ERR_ARG, "shape too large for a kernel test");
    return XSD_OK;
}

int xsd_test_edge_expand(xsd_engine* e, const float* dev_s, long long s_bs, const float* dev_w, int w_last, int flipped, int first_cstride,
                         const float* dev_bias, float* dev_out, const float* dev_mask, float mslope, const unsigned short* dev_bits,
                         int accumulate, float* dev_amax, int B, int H, int W, void* stream)
{
    int rc = edge_hook_args(e, B, H, W);
    if (rc) return rc;
    if (!dev_s || !dev_out || s_bs < 0) return fail(XSD_ERR_ARG, "null image / output plane or negative stride");
    hipStream_t s = (hipStream_t)stream;
    DevMem mem;
    const float* packed = nullptr;
    if ((rc = edge_pack_one(dev_w, w_last, flipped, first_cstride, s, mem, &packed))) return rc;
    EdgeExpandParams p; memset(&p, 0, sizeof(p));
    p.B = B; p.H = H; p.W = W; p.s = dev_s; p.s_bs = s_bs; p.w = packed; p.bias = dev_bias; p.out = dev_out;
    p.mask = dev_mask; p.mslope = mslope; p.bits = dev_bits; p.accumulate = accumulate; p.amax = dev_amax;
    return finish(launch_edge_expand(p, s), s, "edge_expand launch");
}

int xsd_test_edge_reduce(xsd_engine* e, const float* dev_f, const float* dev_w, int w_last, int flipped, int first_cstride,
                         const float* dev_bias, const float* dev_skip, long long skip_bs, float* dev_pre, float* dev_y, long long y_bs,
                         int clamp01, const float* dev_addto, int B, int H, int W, void* stream)
{
    int rc = edge_hook_args(e, B, H, W);
    if (rc) return rc;
    if (!dev_f || !dev_y || skip_bs < 0 || y_bs < 0) return fail(XSD_ERR_ARG, "null feature plane / output or negative stride");
    hipStream_t s = (hipStream_t)stream;
    DevMem mem;
    const float* packed = nullptr;
    if ((rc = edge_pack_one(dev_w, w_last, flipped, first_cstride, s, mem, &packed))) return rc;
    EdgeReduceParams p; memset(&p, 0, sizeof(p));
    p.B = B; p.H = H; p.W = W; p.f = dev_f; p.w = packed; p.bias = dev_bias; p.skip = dev_skip; p.skip_bs = skip_bs;
    p.pre = dev_pre; p.y = dev_y; p.y_bs = y_bs; p.clamp01 = clamp01; p.addto = dev_addto;
    return finish(launch_edge_reduce(p, s), s, "edge_reduce launch");
}

int xsd_test_edge_wgrad(xsd_engine* e, const float* dev_f, const float* dev_s, long long s_bs, int mode, float* dev_dw, float* dev_db,
                        int cstride, int nblocks, int* host_nblocks, int B, int H, int W, void* stream)
{
    int rc = edge_hook_args(e, B, H, W);
    if (rc) return rc;
    if (!dev_f || !dev_s || !dev_dw || !dev_db || s_bs < 0) return fail(XSD_ERR_ARG, "null argument or negative stride");
    if (mode != 0 && mode != 1) return fail(XSD_ERR_ARG, "mode 0 (conv_first) or 1 (conv_last)");
    if (cstride < 9) return fail(XSD_ERR_ARG, "cstride is 9 * in_channels");
    const int rule = edge_wgrad_nblocks();
    if (nblocks < 0 || nblocks > rule) return fail(XSD_ERR_ARG, "at most %d workgroups (the partial-sum buffer)", rule);
    hipStream_t s = (hipStream_t)stream;
    EdgeWgradParams p; memset(&p, 0, sizeof(p));
    p.B = B; p.H = H; p.W = W; p.f = dev_f; p.s = dev_s; p.s_bs = s_bs; p.partial = e->edge_partial; p.nblocks = nblocks ? nblocks : rule;
    if (host_nblocks) *host_nblocks = p.nblocks;
    return finish(launch_edge_wgrad(p, mode, dev_dw, dev_db, s, cstride), s, "edge_wgrad launch");
}

int xsd_test_gconv(int cout, int cin, const float* dev_params, long long param_off, int transposed, const xsd_test_gconv_args* a,
                   int B, int H, int W, int* host_path, void* stream)
{
    int rc = gconv_hook_args(cout, cin, param_off, B, H, W);
    if (rc) return rc;
    if (!dev_params || !a || !a->x || !a->y) return fail(XSD_ERR_ARG, "null argument");
    if (a->shuffle && ((transposed ? cin : cout) & 3)) return fail(XSD_ERR_ARG, "a pixel-shuffled output has a multiple of four channels");
    if (a->e1 && (a->e1c < 0 || a->e1c > (transposed ? cin : cout))) return fail(XSD_ERR_ARG, "e1c lies outside the output channels");
    if (a->skip && a->skipc != 1 && a->skipc != (transposed ? cin : cout)) return fail(XSD_ERR_ARG, "skipc is 1 or the output channel count");
    hipStream_t s = (hipStream_t)stream;
    GenericNet* n = GenericNet::create_convs(1, &cout, &cin, param_off);
    if (!n) return fail(XSD_ERR_NOMEM, "generic-width conv: device allocation failed");
    hipError_t err = n->pack(dev_params, s);
    if (err == hipSuccess) err = n->test_conv(s, 0, transposed != 0, *a, B, H, W);
    rc = finish(err, s, "generic-width conv");
    if (host_path) *host_path = n->last_path;
    delete n;
    return rc;
}

int xsd_test_gwgrad(int cout, int cin, long long param_off, const float* dev_x, long long xbs, const float* dev_g, long long gbs,
                    float* dev_grads, int B, int H, int W, int* host_path, int* host_parts, void* stream)
{
    int rc = gconv_hook_args(cout, cin, param_off, B, H, W);
    if (rc) return rc;
    if (!dev_x || !dev_g || !dev_grads) return fail(XSD_ERR_ARG, "null argument");
    hipStream_t s = (hipStream_t)stream;
    GenericNet* n = GenericNet::create_convs(1, &cout, &cin, param_off);
    if (!n) return fail(XSD_ERR_NOMEM, "generic-width weight gradient: device allocation failed");
    rc = finish(n->test_wgrad(s, 0, dev_x, xbs, dev_g, gbs, B, H, W, dev_grads), s, "generic-width weight gradient");
    if (host_path) *host_path = n->last_path;
    if (host_parts) *host_parts = n->last_parts;
    delete n;
    return rc;
}

int xsd_test_gop(int op, float* dev_d, long long dbs, const float* dev_s, long long sbs, const float* dev_s2, int B, int C, int H, int W,
                 float a, void* stream)
{
    if (op < 0 || op > 5 || !dev_d || !dev_s || B < 1 || C < 1 || H < 1 || W < 1) return fail(XSD_ERR_ARG, "bad op, null argument or empty shape");
    if ((op == 3 || op == 5) && !dev_s2) return fail(XSD_ERR_ARG, "op %d reads a second tensor", op);
    if (op == 3 && (C & 3)) return fail(XSD_ERR_ARG, "the unshuffle writes a multiple of four channels");
    if ((long long)B * C * H * W > (1ll << 28)) return fail(XSD_ERR_ARG, "shape too large for a kernel test");
    hipStream_t s = (hipStream_t)stream;
    const int one = 1;
    GenericNet* n = GenericNet::create_convs(1, &one, &one, 0);
    if (!n) return fail(XSD_ERR_NOMEM, "generic-width op: device allocation failed");
    char what[32];
    snprintf(what, sizeof(what), "generic-width op %d", op);
    const int rc = finish(n->test_op(s, op, dev_d, dbs, dev_s, sbs, dev_s2, B, C, H, W, a), s, what);
    delete n;
    return rc;
}

int xsd_test_gpack(int nconv, const int* host_cout, const int* host_cin, const float* dev_params, float* dev_wt, long long wt_cap,
                   float* dev_wblk, long long wblk_cap, long long* host_off, long long* host_count, void* stream)
{
    if (nconv < 1 || nconv > 8 || !host_cout || !host_cin || !dev_params || !host_off || !host_count) return fail(XSD_ERR_ARG, "bad table or null argument");
    for (int i = 0; i < nconv; ++i)
        if (host_cout[i] < 1 || host_cin[i] < 1 || host_cout[i] > 4096 || host_cin[i] > 4096) return fail(XSD_ERR_ARG, "bad channel counts");
    hipStream_t s = (hipStream_t)stream;
    GenericNet* n = GenericNet::create_convs(nconv, host_cout, host_cin, 0);
    if (!n) return fail(XSD_ERR_NOMEM, "generic-width pack: device allocation failed");
    for (int i = 0; i < nconv; ++i) { host_off[3 * i] = n->convs[i].t; host_off[3 * i + 1] = n->convs[i].pf; host_off[3 * i + 2] = n->convs[i].pt; }
    host_count[0] = n->wt_floats; host_count[1] = n->wblk_floats;
    if ((dev_wt && wt_cap < n->wt_floats) || (dev_wblk && wblk_cap < n->wblk_floats)) { delete n; return fail(XSD_ERR_ARG, "a read-back buffer is too small"); }
    hipError_t err = n->pack(dev_params, s);
    if (err == hipSuccess && dev_wt) err = hipMemcpyAsync(dev_wt, n->wt, sizeof(float) * n->wt_floats, hipMemcpyDeviceToDevice, s);
    if (err == hipSuccess && dev_wblk && n->wblk_floats) err = hipMemcpyAsync(dev_wblk, n->wblk, sizeof(float) * n->wblk_floats, hipMemcpyDeviceToDevice, s);
    const int rc = finish(err, s, "generic-width pack");
    delete n;
    return rc;
}

// ---- the loss kernels scale by scale, the pooling and the plane path's clamp backward (include/xsd.h) ----
int xsd_loss_test_scale(const xsd_loss_config* cfg, const float* dev_y, const float* dev_target, const float* dev_gup, const float* dev_coarse,
                        float* dev_dy, int accumulate, double* dev_stat, float* host_scal11, int B, int H, int W, void* stream)
{
    if (!cfg || !dev_y || !dev_target || !dev_stat || !host_scal11) return fail(XSD_ERR_ARG, "null argument");
    if (!(cfg->sigma > 0.f)) return fail(XSD_ERR_ARG, "loss: sigma must be > 0");
    if ((dev_dy != nullptr) != (dev_gup != nullptr)) return fail(XSD_ERR_ARG, "dy and the upstream pair come together");
    if (dev_coarse && !dev_dy) return fail(XSD_ERR_ARG, "a coarse gradient needs dy");
    LossWeights w;
    for (int i = 0; i < 5; ++i) w.w[i] = 0.f;
    w.w[3] = 1.f;                                  // what loss_check refuses for ssim
    w.correction = 0.f; w.sigma = cfg->sigma; w.k1 = cfg->k1; w.k2 = cfg->k2; w.kernel_size = cfg->kernel_size;
    const char* why = nullptr;
    if (loss_check(w, B, H, W, &why)) return fail(XSD_ERR_ARG, "%s", why);
    if ((long long)B * H > 0x7fffffffll / W) return fail(XSD_ERR_ARG, "shape too large for a kernel test");
    hipError_t err = loss_test_scale(w, dev_y, dev_target, dev_gup, dev_coarse, dev_dy, accumulate, dev_stat, host_scal11, B, H, W, (hipStream_t)stream);
    if (err != hipSuccess) return fail(XSD_ERR_HIP, "loss scale: %s", hipGetErrorString(err));      // (synchronous by itself: xsd_loss.h)
    return XSD_OK;
}

int xsd_loss_test_pool2(const float* dev_p, const float* dev_t, float* dev_po, float* dev_to, int B, int H, int W, void* stream)
{
    if (!dev_p || !dev_t || !dev_po || !dev_to || B < 1 || H < 2 || W < 2) return fail(XSD_ERR_ARG, "null argument or an image under 2 x 2");
    if ((long long)B * H > 0x7fffffffll / W) return fail(XSD_ERR_ARG, "shape too large for a kernel test");
    hipStream_t s = (hipStream_t)stream;
    return finish(loss_test_pool2(dev_p, dev_t, dev_po, dev_to, B, H, W, s), s, "pool2");
}

int xsd_test_clamp_bwd(const float* dev_pre, const float* dev_dy, float* dev_dpre, int64_t n, void* stream)
{
    if (!dev_pre || !dev_dy || !dev_dpre || n <= 0) return fail(XSD_ERR_ARG, "null argument or n <= 0");
    hipStream_t s = (hipStream_t)stream;
    return finish(launch_clamp_bwd(dev_pre, dev_dy, dev_dpre, n, s), s, "clamp backward");
}

int xsd_test_packed_region(xsd_engine* e, int region, void* dev_dst, int64_t dst_bytes, int64_t* info, void* stream)
{
    if (!e || !info) return fail(XSD_ERR_ARG, "null argument");
    if (e->generic) return fail(XSD_ERR_ARG, "xsd_test_packed_region: a generic-width engine has no plane panels");
    if (region < 0 || region >= XSD_PACKED_REGIONS) return fail(XSD_ERR_ARG, "xsd_test_packed_region: unknown region %d", region);
    if (!e->packed) return fail(XSD_ERR_STATE, "xsd_test_packed_region needs a preceding xsd_pack_weights");
    const int ci = e->cfg.in_channels, co = e->cfg.out_channels, nup = (int)e->up.size();
    const void* src = nullptr;
    int64_t bytes = 0;
    std::vector<int64_t> table;
    switch (region) {
    case XSD_PACKED_PK_FWD: src = e->pk_fwd; bytes = 4 * e->pk_floats; break;
    case XSD_PACKED_PK_BWD: src = e->pk_bwd; bytes = 4 * e->pk_floats; break;
    case XSD_PACKED_PK_FWD_S: src = e->pk_fwd_s; bytes = 4 * e->pk_floats; break;
    case XSD_PACKED_PK_BWD_S: src = e->pk_bwd_s; bytes = 4 * e->pk_floats; break;
    case XSD_PACKED_AMAX: src = e->amax; bytes = 2 * 4; break;
    case XSD_PACKED_PK_EDGE: src = e->pk_edge; bytes = 4ll * 2 * 288 * e->planes * (ci + co); break;
    case XSD_PACKED_PK_SBIAS: src = e->pk_sbias; for (auto& c : e->up) bytes += 4ll * c.cout; break;
    case XSD_PACKED_PARAMS_PAD: src = e->params_pad; bytes = e->nf_pad ? 4 * e->nparams_pad : 0; break;
    default: {  // XSD_PACKED_TABLE: the descriptors the pack kernels read, copied back from the device
        std::vector<PackDesc> descs(e->ndesc);
        HIPCHK(hipMemcpy(descs.data(), e->descs_dev, sizeof(PackDesc) * descs.size(), hipMemcpyDeviceToHost));
        table = {e->ndesc, nup, e->first_w, e->last_w, e->planes, e->nf_pad, e->pk_floats, e->nf_pad ? e->nparams_pad : e->nparams};
        for (auto& d : descs) {
            unsigned int bits; memcpy(&bits, &d.bwd_scale, 4);
            table.insert(table.end(), {d.src_w, d.dst_fwd, d.dst_bwd, d.cout, d.cin, d.shuffle, (int64_t)bits});
        }
        for (auto& c : e->up) table.insert(table.end(), {c.b_off, c.sbias_off});
        bytes = 8 * (int64_t)table.size();
    } }
    info[0] = bytes;
    if (!dev_dst) return XSD_OK;
    if (dst_bytes < bytes) return fail(XSD_ERR_ARG, "xsd_test_packed_region: region %d holds %lld bytes, the buffer %lld", region, (long long)bytes, (long long)dst_bytes);
    if (bytes == 0) return XSD_OK;
    if (region == XSD_PACKED_TABLE) { memcpy(dev_dst, table.data(), (size_t)bytes); return XSD_OK; }
    hipStream_t s = (hipStream_t)stream;
    char what[32];
    snprintf(what, sizeof(what), "packed region %d", region);
    return finish(hipMemcpyAsync(dev_dst, src, (size_t)bytes, hipMemcpyDeviceToDevice, s), s, what);
}

int xsd_test_pad_gather(xsd_engine* e, float* dev_grads_real, const float* dev_grads_padded, void* stream)
{
    if (!e || !dev_grads_real || !dev_grads_padded) return fail(XSD_ERR_ARG, "null argument");
    if (e->generic || !e->nf_pad) return fail(XSD_ERR_ARG, "xsd_test_pad_gather: the engine's width is not zero-padded");
    hipStream_t s = (hipStream_t)stream;
    return finish(launch_pad_params(dev_grads_real, const_cast<float*>(dev_grads_padded), static_cast<const PadDesc*>(e->pad_descs), e->npad, 1, s), s, "pad gather");
}

int xsd_test_add_channels(float* dev_dst, const float* dev_src, int C, int64_t HW, int B, void* stream)
{
    if (!dev_dst || !dev_src || C < 1 || HW < 1 || B < 1) return fail(XSD_ERR_ARG, "null argument or an extent < 1");
    hipStream_t s = (hipStream_t)stream;
    return finish(launch_add_channels(dev_dst, dev_src, C, HW, B, s), s, "add channels");
}

// ---- the device-memory ledger (xsd_mem.h) ------------------------------------------------------------------------
int xsd_test_mem_stats(int64_t* out, int n)
{
    if (!out || n < 1 || n > 6) return fail(XSD_ERR_ARG, "xsd_test_mem_stats: null out or n outside 1..6");
    int64_t all[6];
    xsd::mem_stats(all);
    memcpy(out, all, sizeof(int64_t) * n);
    return XSD_OK;
}

int64_t xsd_test_mem_refuse(int64_t nth) { return xsd::mem_refuse(nth); }

} // extern "C"
