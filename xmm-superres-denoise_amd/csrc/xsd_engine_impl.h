// xsd_engine_impl.h -- what xsd_engine.hip (the engine and the C ABI) and xsd_test_entries.hip (the kernel-level test entries) share:
// the engine's state, the view arithmetic of a feature plane, the max-|x| slots the test entries borrow, and the functions both the
// plan and a test entry call, so that an entry cannot drift from the plan.  Each function has its one definition in xsd_engine.hip
// and hidden visibility: none of them is a dynamic symbol of the library.  Nothing here depends on XSD_TEST_HOOKS or XSD_DIAG.
// Include it last: `fail` is a macro.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <functional>
#include <vector>

#include "../../include/xsd.h"
#include "xsd_aux.h"
#include "xsd_err.h"
#include "xsd_mem.h"
#include "generic_net.h"

using namespace xsd;

#define fail xsd::failf
#define HIPCHK(expr)                                                                                      \
    do {                                                                                                  \
        hipError_t _e = (expr);                                                                           \
        if (_e != hipSuccess) return fail(XSD_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

struct ConvW {       // one MFMA conv's weights
    long long w_off, b_off; // flat-param offsets
    int cout, cin, shuffle;
    long long fwd_off, bwd_off; // packed offsets (floats)
    long long sbias_off;        // shuffled-bias offset (shuffle convs) or -1
    float bwd_scale = 1.f;      // folded into the input-gradient panels
};

typedef std::function<hipError_t(hipStream_t)> Launch;

struct ProfRec { hipEvent_t a, b; double flop, bytes; int klass; };

struct xsd_engine {
    xsd_config cfg;
    GenericNet* generic = nullptr;   // what the plane kernels do not take (generic_net.hip): more than 256 filters, more than 8 image channels
    // Widths that are no multiple of 32 run zero-padded to the next one: the engine is built for `nf_pad` filters over an internal,
    // padded flat parameter vector (pad weights and biases 0 -> pad channels are exactly 0 everywhere, forward and backward); the
    // caller's vectors keep the reference's layout for `cfg.num_filters` (pad_params_kernel expands, pad_grads_kernel gathers)
    int nf_pad = 0;                  // 0: no padding
    long long nparams_pad = 0;
    float* params_pad = nullptr;
    float* grads_pad = nullptr;
    void* pad_descs = nullptr;       // PadDesc[npad]: first | dense blocks | trunk, last, up.., hr  (= backward stages last | 1..blocks | 0)
    int npad = 0;
    std::vector<long long> rrdb_begin_real;
    long long nparams_real = 0;
    int planes = 1;                  // num_filters / 32: 32-channel planes per feature tensor (1 = the shipped configuration; up to 8: Builder::build)
    long long nparams = 0;
    // flat-param offsets
    long long first_w = 0, first_b = 0, last_w = 0, last_b = 0;
    std::vector<ConvW> rdb; // blocks*15
    ConvW trunk, hr;
    std::vector<ConvW> up;
    std::vector<long long> rrdb_begin; // flat offset where rrdb.i starts; [blocks] = trunk offset
    // packed weights
    float* pk_fwd = nullptr;
    float* pk_bwd = nullptr;
    unsigned short* pk_fwd_s = nullptr; // split-mode panels (mode 3: fp32 in bf16-MFMA fragment order; mode 4: two-term fp16 images),
    unsigned short* pk_bwd_s = nullptr; // same byte size / offsets as pk_fwd / pk_bwd
    int chunk = 0;             // diagnostic library only (env XSD_CHUNK): images per dense-block sweep (0 = whole batch)
    int ablate = 0;            // diagnostic library only (env XSD_ABLATE): ablation knobs of the kernels
    int math = 4;              // include/xsd.h: xsd_set_math (default: f16x3, the faster of the two fp32-class split modes)
    float* pk_edge = nullptr; // first_fwd, first_bwd, last_fwd, last_bwd (288 each)
    float* pk_sbias = nullptr;
    PackDesc* descs_dev = nullptr;
    int ndesc = 0;
    long long pk_floats = 0;
    // math mode 4 (f16x3): max |x| slots; [0] packed forward panels, [1] packed input-gradient panels, [2..] planes of the plan
    float* amax = nullptr;
    int amax_used = 2;
    int amax_bwd_first = 2;    // first slot the plan hands out while it builds the BACKWARD stages (re-zeroed by stage 0 of every backward)
    int ncu = 256;             // compute units of the device the engine was created on (the weight gradient's block launch is dealt from it)
    int amax_cap = 65536;      // floats allocated behind `amax`; ensure_plan grows it to what the plan's sizing pass counted (+ AMAX_TAIL)
    static constexpr int AMAX_TAIL = 64;   // the last slots belong to the single-launch test entries: TestSlots below
    const float* params = nullptr; // borrowed (bias reads)
    bool packed = false;
    // workspace
    char* ws = nullptr;
    size_t ws_bytes = 0;
    float* wg_partial = nullptr;
    float* wg_bias_partial = nullptr;
    float* edge_partial = nullptr;
    double* loss_partial = nullptr;
    int nparts = 256;
    // plan
    int pB = 0, pH = 0, pW = 0, ptrain = -1;
    std::vector<Launch> fwd_ops;
    std::vector<std::vector<Launch>> bwd_stages;
    bool fwd_saved = false;
    // late-bound call pointers
    const float* b_x = nullptr;
    float* b_y = nullptr;
    const float* b_dy = nullptr;
    float* b_dx = nullptr;
    float* b_grads = nullptr;
    void* zero_page = nullptr;         // 256 B of zeros (padding source of the DMA / unconditional loads) + 256 B of trash
    unsigned long long* dbg = nullptr; // conv phase stamps (diagnostic)
    // profiling
    bool prof = false;
    std::vector<ProfRec> recs;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
};

// The max-|x| slots a single-launch test entry borrows (math mode 4: nobody has reported its operands' maxima), as distances below the
// end of the slot array.  The plan's own slots stop AMAX_TAIL short of the end (Builder::new_slot), so no plan launch ever meets one.
struct TestSlots {
    enum { IN = 32, OUT = 24, X = 16, G = 11, W_FWD = 4, W_BWD = 3 };
    float *in, *out;       // a conv launch: its input planes, its output chunks            (five slots each)
    float *x, *g;          // a weight-gradient launch: its X planes, its G planes          (five slots each)
    float *w_fwd, *w_bwd;  // the single-conv packer: max |w| of the forward and of the input-gradient panels (adjacent: pack_panels' amax2)
    static_assert(IN <= xsd_engine::AMAX_TAIL && IN - 5 >= OUT && OUT - 5 >= X && X - 5 >= G && G - 5 >= W_FWD && W_FWD - 1 == W_BWD && W_BWD >= 1,
                  "the borrowed slots lie inside the tail of the slot array, in ranges that do not overlap");
};
inline TestSlots test_slots(const xsd_engine* e)
{
    float* end = e->amax + e->amax_cap;
    return {end - TestSlots::IN, end - TestSlots::OUT, end - TestSlots::X, end - TestSlots::G, end - TestSlots::W_FWD, end - TestSlots::W_BWD};
}

// View arithmetic of the feature planes of a B x H x W batch (`level`: the plane holds (H << level) x (W << level) pixels): the parameter
// blocks' shape fields and the standard / pixel-shuffled views.  The plan Builder derives from it; the test entries use it as it is.
struct PlaneViews {
    int B, H, W;
    ConvParams conv_base(int level) const
    {
        ConvParams p;
        memset(&p, 0, sizeof(p));
        p.B = B; p.H = H << level; p.W = W << level;
        p.tilesX = (p.W + TILE_W - 1) / TILE_W;
        p.tilesY = (p.H + TILE_H - 1) / TILE_H;
        p.std_rs = p.W * 32;
        p.std_bs = (long long)p.H * p.W * 32;
        for (int j = 0; j < 5; ++j) { p.out[j].a1 = 1.f; p.out[j].a2 = 1.f; p.out[j].slope = 1.f; p.out[j].mslope = 1.f; }
        return p;
    }
    WgradParams wgrad_base(int level) const
    {
        WgradParams wp;
        memset(&wp, 0, sizeof(wp));
        wp.B = B; wp.H = H << level; wp.W = W << level;
        wp.tilesX = (wp.W + TILE_W - 1) / TILE_W;
        wp.tilesY = (wp.H + TILE_H - 1) / TILE_H;
        return wp;
    }
    PlaneIn std_in(const float* p, int level) const
    {
        PlaneIn r; r.p = p; r.ps = 32; r.rs = (W << level) * 32; r.bs = (long long)(H << level) * (W << level) * 32; return r;
    }
    // sub-pixel (i,j) view at `level` of a plane stored at level+1 (PixelShuffle(2), generator_rrdb.py:97)
    PlaneIn shuf_in(const float* hr, int level, int n) const
    {
        const int Wl = W << level, Hl = H << level;
        PlaneIn r; r.p = hr + ((long long)(n >> 1) * 2 * Wl + (n & 1)) * 32; r.ps = 64; r.rs = 4 * Wl * 32;
        r.bs = (long long)4 * Hl * Wl * 32; return r;
    }
    void std_out(OutDesc& o, float* p, int level) const
    {
        o.p = p; o.ps = 32; o.rs = (W << level) * 32; o.bs = (long long)(H << level) * (W << level) * 32;
    }
    void shuf_out(OutDesc& o, float* hr, int level, int n) const
    {
        PlaneIn r = shuf_in(hr, level, n);
        o.p = const_cast<float*>(r.p); o.ps = r.ps; o.rs = r.rs; o.bs = r.bs;
    }

    // the same conv restricted to images [b0, b0 + nb)
    static ConvParams slice(const ConvParams& q, int b0, int nb)
    {
        ConvParams p = q;
        p.B = nb;
        for (int i = 0; i < 5; ++i) if (p.in[i].p) p.in[i].p += (long long)b0 * p.in[i].bs;
        for (int j = 0; j < 5; ++j) {
            OutDesc& o = p.out[j];
            if (o.p) o.p += (long long)b0 * o.bs;
            if (o.e1) o.e1 += (long long)b0 * p.std_bs;
            if (o.e2) o.e2 += (long long)b0 * p.std_bs;
            if (o.e3) o.e3 += (long long)b0 * p.std_bs;
            if (o.mask) o.mask += (long long)b0 * p.std_bs;
            if (o.bits_out) o.bits_out += (long long)b0 * (p.std_bs / 16);   // 2 half-words per pixel of 32 floats
            if (o.bits_in) o.bits_in += (long long)b0 * (p.std_bs / 16);
        }
        return p;
    }
};

struct PadDesc {
    long long w_r, b_r, w_p, b_p;    // weight / bias offsets in the caller's (real) and in the padded flat vector
    int cout_r, cin_r, cin_p;        // OIHW extents (cout_p never matters: output channel oc keeps its index)
    int tin_r, tin_p;                // width of the tensors the input is concatenated from: input channel t*tin_r + k <-> t*tin_p + k
};

struct WgradBlock {
    WgradParams wp;               // the pair-list launch; the caller sets the planes, their max-|x| slots and the late-bound pointers
    WgradReduceParams rp[5];      // conv n + 1's reduction; the caller sets dw and db
};

// Profile classes of xsd_profile_read (include/xsd.h): 0 conv (forward + input-gradient), 1 weight gradient; the HBM-bound kernels:
// 2 edge_expand (1 -> 32), 3 edge_reduce (32 -> 1), 4 edge_wgrad, 5 L1 loss, 6 Adam, 7 clamp backward, 8 plane max |x| sweeps.
// `bytes` is ALGORITHMIC traffic (SURVEY 8d rule: every operand once), `flop` 2 x MAC.
enum { PK_CONV = 0, PK_WGRAD = 1, PK_EDGE_EXPAND = 2, PK_EDGE_REDUCE = 3, PK_EDGE_WGRAD = 4, PK_LOSS = 5, PK_ADAM = 6, PK_CLAMP_BWD = 7, PK_PLANE_AMAX = 8, PK_COUNT = 9 };

#pragma GCC visibility push(hidden)
hipError_t launch_wgrad_split(int math, int ablate, const WgradParams& p, hipStream_t s);
int wgrad_nparts(const xsd_engine* e, int n_in, int n_g);
int wgrad_block_nparts(const xsd_engine* e);
void wgrad_block_fill(WgradBlock& k, int nparts, const int cin[5], const int cout[5], float gscale, float* partial, float* bias_partial);
hipError_t wgrad_block_reduce(const WgradBlock& k, bool separate, hipStream_t s);
int edge_wgrad_nblocks();
hipError_t launch_conv_any(xsd_engine* eng, ConvParams& p, hipStream_t s);
// the zero-padded widths' expansion (to_real 0: caller's parameters -> padded vector) or gather (1: padded gradients -> caller's vector) of `ndesc` convs
hipError_t launch_pad_params(const float* real, float* padded, const PadDesc* descs_dev, int ndesc, int to_real, hipStream_t s);
// OIHW weights -> the panels of math mode `math`: the whole net (xsd_pack_weights) or one conv (the test entries' packer)
hipError_t pack_panels(int math, const float* dev_params, const PackDesc* descs_dev, int ndesc, float* pk_fwd, float* pk_bwd,
                       void* pk_fwd_s, void* pk_bwd_s, long long pk_floats, float* amax2, hipStream_t s);
#pragma GCC visibility pop
