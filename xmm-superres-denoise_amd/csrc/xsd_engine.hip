// xsd_engine.hip -- host side of the engine: network plan (forward / backward launch schedules over feature planes),
// workspace, weight packing, and the C ABI declared in include/xsd.h (its kernel-level test entries: xsd_test_entries.hip, over xsd_engine_impl.h).
//
// The schedule restates, layer by layer, the reference graph
//   _GeneratorRRDB.forward / GeneratorRRDB_SR.forward / GeneratorRRDB_DN.forward (generator_rrdb.py:66-69,103-110,130-137)
//   RRDB.forward / ResidualDenseBlock_5C.forward                                   (rrdb_blocks.py:37-54,66-70)
//   Model.forward's second clamp                                                   (models/model.py:48-49)
// and its reverse-mode derivative (what torch autograd would run), with every elementwise op fused into the epilogue
// of the conv that produces its operand.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <tuple>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <new>
#include <vector>

#include "xsd_loss.h"
#include "xsd_engine_impl.h"

static constexpr int EDGE_WGRAD_BLOCKS = 2048; // 8 workgroups of 256 threads per CU

namespace xsd {
int debug_conv_occupancy(int lds_bytes);
float debug_residency_ms(int grid, int threads, int lds_bytes, int us);
hipError_t probe_mfma_stream(int fmt, double seconds, double* mfma_tflops, double* sclk_ghz, hipStream_t stream);
hipError_t launch_pack_shuffle_bias(const float* b, float* out, int planes, hipStream_t s);
}

static thread_local std::string g_err;
namespace xsd {
int failf(int code, const char* fmt, ...)      // xsd_err.h: every translation unit of the library reports through here
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
} // namespace xsd

// ------------------------------------------------------------------------------------------------------------
static void take_conv(long long& off, int cout, int cin, long long& w, long long& b)
{
    w = off; off += (long long)cout * cin * 9;
    b = off; off += cout;
}

// weight gradient of the split modes: mode 3 (bf16x6) and mode 4 (f16x3) have their own role-split kernels (one workgroup
// per CU, `nparts` partial sums); diagnostic ablate bit 22 runs mode 3's kernel in mode 4
hipError_t launch_wgrad_split(int math, int ablate, const WgradParams& p, hipStream_t s)
{
    return (math == 4 && !(ablate & (1 << 22))) ? launch_wgrad_h2x(p, s) : launch_wgrad_s3x(p, s);
}

// Parts (partial sums) of one weight-gradient launch over the n_in x n_g rectangle: the plan (Builder::wgrad_launch) and the single-launch
// test hook (xsd_test_wgrad_ex) both ask here, so the hook cannot drift from the plan.
int wgrad_nparts(const xsd_engine* e, int n_in, int n_g)
{
#ifndef XSD_WGRAD_ROUNDS
    // The grid is nparts x n_in x n_g workgroups of one per CU: with nparts = the CU count a launch over k (X, G) pairs runs k
    // rounds of workgroups, and every round pays a workgroup's fixed cost again (first two tiles' round trips, the final
    // LDS reduction and partial-sum store, ~30 us of a ~450 us round: kernel trace, 0.476 / 0.911 / 1.359 / 1.731 / 2.250 ms
    // for 1..5 pairs).  Where the pairs divide the CUs into a multiple of eight parts (2 and 4 pairs: 128 / 64 parts) the whole
    // launch is ONE round of k-times longer workgroups; the workgroups that share G tiles still run side by side on one XCD.
    // 3 and 5 pairs would leave 16 CUs idle (240 workgroups): they keep the k rounds.
    const int pairs = n_in * n_g;
    if (e->math >= 3 && pairs > 1 && e->nparts % pairs == 0 && ((e->nparts / pairs) & 7) == 0) return e->nparts / pairs;   // (the split modes' kernels: one workgroup per CU; the exact-fp32 kernel runs two)
#endif
    return e->nparts;
}

// A dense block's FIFTEEN (X_j, G_n) pairs (conv n + 1 reads x_0 .. x_n: j <= n) as ONE pair-list launch (Builder::wgrad_block_launch)
// plus the five convs' reductions.  The plan and the block test hook (xsd_test_wgrad_block) both fill their launch here, so the hook
// cannot drift from the plan: the part count, the pair list, where each conv's panels and bias sums start, the strides, the scales.
// m parts per XCD, each 15 workgroups side by side: m = CUs / (8 x 15), at most 10 ((8 m + 1) x 15 partial panels must fit
// wg_partial's 256 x 5); m = 0 (fewer than 120 CUs): the plan runs one launch per G instead
static int block_parts_per_xcd(int ncu) { const int m = ncu / 120; return m > 10 ? 10 : m; }
int wgrad_block_nparts(const xsd_engine* e)
{
    // (MI355X: 256 CUs -> 16 parts = 240 workgroups; the kernel's decode takes any nparts = 8 m or 8 m + 1)
    const int m = block_parts_per_xcd(e->ncu);
    // one more part on the CUs the 8 m x 15 workgroups leave, when those can hold its 15 slots two per XCD (>= 16 spare CUs;
    // MI355X: exactly 16): no L2 sharing for it, no idle CU
    // (XSD_WGRAD_TAIL=0 (include/xsd.h): 8 m parts; same device 124.7 -> 125.2 tiles/s, the kernel -1.9 %)
#ifdef XSD_TEST_HOOKS      // only the hooks variant of the library (make hooks; include/xsd.h) reads the environment here
    static const int tail = getenv("XSD_WGRAD_TAIL") ? atoi(getenv("XSD_WGRAD_TAIL")) : 1;
#else
    constexpr int tail = 1;
#endif
    return (tail && e->ncu - 120 * m >= 16) ? 8 * m + 1 : 8 * m;
}
// `k.wp` comes from Builder::wgrad_base; cin[n], cout[n]: the OIHW extent of conv n + 1's gradient; gscale: conv 5's factor
void wgrad_block_fill(WgradBlock& k, int nparts, const int cin[5], const int cout[5], float gscale, float* partial, float* bias_partial)
{
    WgradParams& wp = k.wp;
    wp.n_in = 5; wp.n_g = 5; wp.nparts = nparts; wp.npairs = 15;
    wp.partial = partial; wp.bias_partial = bias_partial;
    // slots are conv-major (conv 5 first), so conv n's blocks are contiguous and each conv gets its own fixed-order reduce
    int first[5], slot = 0;
    wp.pair_j = 0; wp.pair_n = 0;
    for (int n = 4; n >= 0; --n) {
        first[n] = slot;
        for (int j = 0; j <= n; ++j, ++slot) { wp.pair_j |= (unsigned long long)j << (4 * slot); wp.pair_n |= (unsigned long long)n << (4 * slot); }
    }
    for (int n = 0; n < 5; ++n) {
        WgradReduceParams& r = k.rp[n];
        memset(&r, 0, sizeof(r));
        r.nparts = nparts; r.n_in = n + 1; r.n_g = 1; r.cin_total = cin[n]; r.cout_total = cout[n];
        r.shuffle = 0; r.scale = n == 4 ? gscale : 1.f;
        r.part_stride = (long long)wp.npairs * PANEL_FLOATS; r.bias_stride = wp.n_g * 32;
        r.partial = partial + (long long)first[n] * PANEL_FLOATS; r.bias_partial = bias_partial + n * 32;
    }
}
// the five convs' fixed-order reductions as one launch (bitwise what five launches give: `separate`, the test hook's other form)
hipError_t wgrad_block_reduce(const WgradBlock& k, bool separate, hipStream_t s)
{
    if (separate) {
        for (int n = 0; n < 5; ++n) { hipError_t err = launch_wgrad_reduce(k.rp[n], s); if (err != hipSuccess) return err; }
        return hipSuccess;
    }
    WgradReduceBatch rb;
    memset(&rb, 0, sizeof(rb));
    rb.n = 5;
    for (int n = 0; n < 5; ++n) rb.r[n] = k.rp[n];
    return launch_wgrad_reduce_multi(rb, s);
}

// Workgroups (partial sums) of one edge weight-gradient launch: the plan and the single-launch test hook (xsd_test_edge_wgrad) both ask
// here.  A constant: the kernel strides over the image rows, idle workgroups store zeros, edge_partial holds this many records.
int edge_wgrad_nblocks() { return EDGE_WGRAD_BLOCKS; }

static hipError_t prof_launch(xsd_engine* e, int klass, double flop, double bytes, hipStream_t s, const std::function<hipError_t()>& f)
{
    if (!e->prof) return f();
    auto get_ev = [&]() -> hipEvent_t {
        if (e->ev_used == e->ev_pool.size()) {
            hipEvent_t ev;
            if (hipEventCreate(&ev) != hipSuccess) return nullptr;
            e->ev_pool.push_back(ev);
        }
        return e->ev_pool[e->ev_used++];
    };
    ProfRec r{get_ev(), get_ev(), flop, bytes, klass};
    if (!r.a || !r.b) return hipErrorOutOfMemory;
    hipEventRecord(r.a, s);
    hipError_t err = f();
    hipEventRecord(r.b, s);
    e->recs.push_back(r);
    return err;
}

// conv launch of the engine's math mode (mode 4 also needs the weight buffers' max |w| slot: forward or input-gradient panels)
hipError_t launch_conv_any(xsd_engine* eng, ConvParams& p, hipStream_t s)
{
    if (eng->math == 4) {
        if (!p.amax_w) {
            const float* lo = reinterpret_cast<const float*>(eng->pk_fwd_s);
            p.amax_w = (p.wstep[0] >= lo && p.wstep[0] < lo + eng->pk_floats) ? eng->amax + 0 : eng->amax + 1;
        }
        return launch_conv3x3_h2x(p, s);
    }
    return eng->math == 3 ? launch_conv3x3_s3x(p, s) : launch_conv3x3_mfma(p, s);
}

static hipError_t run_edge_expand(xsd_engine* e, const EdgeExpandParams& p, hipStream_t s)
{
    const double px = (double)p.B * p.H * p.W;      // reads the image (4 B/px), writes the plane (128); + the plane it adds to; + the mask plane or its compact words
    const double bytes = px * (4.0 + 128.0 + (p.accumulate ? 128.0 : 0.0) + (p.bits ? 4.0 : (p.mask ? 128.0 : 0.0)));
    return prof_launch(e, PK_EDGE_EXPAND, 2.0 * 9 * 32 * px, bytes, s, [&]() { return launch_edge_expand(p, s); });
}
static hipError_t run_edge_reduce(xsd_engine* e, const EdgeReduceParams& p, hipStream_t s)
{
    const double px = (double)p.B * p.H * p.W;      // reads the plane (128 B/px) (+ skip, + addto), writes y (+ pre)
    const double bytes = px * (128.0 + 4.0 + (p.skip ? 4.0 : 0.0) + (p.addto ? 4.0 : 0.0) + (p.pre ? 4.0 : 0.0));
    return prof_launch(e, PK_EDGE_REDUCE, 2.0 * 9 * 32 * px, bytes, s, [&]() { return launch_edge_reduce(p, s); });
}
static hipError_t run_edge_wgrad(xsd_engine* e, const EdgeWgradParams& p, int which, float* dw, float* db, hipStream_t s, int cstride = 9)
{
    const double px = (double)p.B * p.H * p.W;      // reads the plane and the image once
    return prof_launch(e, PK_EDGE_WGRAD, 2.0 * 9 * 32 * px, px * (128.0 + 4.0), s, [&]() { return launch_edge_wgrad(p, which, dw, db, s, cstride); });
}

// ------------------------------------------------------------------------------------------------------------
// Plan builder
// ------------------------------------------------------------------------------------------------------------
struct Builder : PlaneViews {
    xsd_engine* e;
    bool train;
    uintptr_t base;      // 0 in the sizing pass
    size_t top = 0, peak = 0;
    std::vector<std::vector<size_t>> freelist; // per level
    // math mode 4 (f16x3): which plane views have a slot holding their max |x| (set by the producing conv's epilogue or by
    // a plane_amax launch in front of the first consumer); a view dies when its buffer is handed out again
    typedef std::vector<float*> Tensor;      // a feature tensor: num_filters / 32 planes of 32 channels, in torch.cat's channel order
    typedef std::tuple<uintptr_t, int, int> ViewKey;
    std::map<ViewKey, float*> amax_valid;
    Builder(xsd_engine* e_, int B_, int H_, int W_, bool train_, uintptr_t base_)
        : PlaneViews{B_, H_, W_}, e(e_), train(train_), base(base_), freelist(8) {}

    float* new_slot()
    {
        // one slot per plane view a launch writes or reads first.  The sizing pass of ensure_plan only COUNTS (a deep, wide net
        // needs more than the initial allocation: 256 filters x 64 blocks is ~80k); the real pass runs after the array has
        // been grown to the count, so no two planes ever share a slot
        const int i = e->amax_used++;
        return (e->amax && i < e->amax_cap - xsd_engine::AMAX_TAIL) ? e->amax + i : nullptr;
    }
    void invalidate_range(uintptr_t lo, size_t bytes)
    {
        for (auto it = amax_valid.begin(); it != amax_valid.end();) {
            const uintptr_t k = std::get<0>(it->first);
            if (k >= lo && k < lo + bytes) it = amax_valid.erase(it); else ++it;
        }
    }
    // a producer outside the conv kernels (edge_expand) reports the max |x| of the standard plane it writes
    float* report_slot(float* plane, int level)
    {
        if (e->math != 4) return nullptr;
        const PlaneIn v = std_in(plane, level);
        invalidate_range(reinterpret_cast<uintptr_t>(plane), plane_bytes(level));
        float* slot = new_slot();
        amax_valid[ViewKey(reinterpret_cast<uintptr_t>(v.p), v.rs, v.ps)] = slot;
        return slot;
    }
    // slot of an input view; if nobody has reported it yet, `pre` gets the reduction launch
    float* slot_of(const PlaneIn& v, int Hv, int Wv, std::vector<Launch>& pre)
    {
        const ViewKey key(reinterpret_cast<uintptr_t>(v.p), v.rs, v.ps);
        auto it = amax_valid.find(key);
        if (it != amax_valid.end()) return it->second;
        float* slot = new_slot();
        amax_valid[key] = slot;
        const int Bv = B;
        xsd_engine* eng = e;
        pre.push_back([eng, v, Bv, Hv, Wv, slot](hipStream_t s) { return prof_launch(eng, PK_PLANE_AMAX, 0.0, 128.0 * Bv * Hv * Wv, s, [&]() { return launch_plane_amax(v, Bv, Hv, Wv, slot, s); }); });
        return slot;
    }

    // The ONE launch that wrote the four pixel-shuffled views of a high-resolution plane published ONE maximum -- over all of its
    // output chunks (conv3x3_h2x.hip: run_max) -- into each view's slot: that number IS the plane's max |x|, so the standard view
    // of the plane (what HRconv and the weight gradient read) takes view 0's slot instead of a plane_amax sweep over 4 x the
    // low-resolution pixels (round 6: 2.7 % of a batch-1 SR forward, 0.8 % at batch 16; results identical by construction)
    void alias_shuffled(float* hr, int level)
    {
        if (e->math != 4) return;
        OutDesc o; memset(&o, 0, sizeof(o));
        shuf_out(o, hr, level, 0);
        auto it = amax_valid.find(ViewKey(reinterpret_cast<uintptr_t>(o.p), o.rs, o.ps));
        if (it == amax_valid.end()) return;
        const PlaneIn v = std_in(hr, level + 1);
        amax_valid[ViewKey(reinterpret_cast<uintptr_t>(v.p), v.rs, v.ps)] = it->second;
    }

    size_t plane_bytes(int level, int ch = 32) const
    {
        return ((size_t)B * (H << level) * (W << level) * ch * sizeof(float) + 255) & ~(size_t)255;
    }
    float* alloc(int level)
    {
        size_t off;
        if (!freelist[level].empty()) { off = freelist[level].back(); freelist[level].pop_back(); }
        else { off = top; top += plane_bytes(level); if (top > peak) peak = top; }
        if (e->math == 4) invalidate_range(base + off, plane_bytes(level));
        return reinterpret_cast<float*>(base + off);
    }
    float* alloc_img(int level, int ch) // ch-channel image [B][ch][H][W]
    {
        size_t off = top; top += plane_bytes(level, ch); if (top > peak) peak = top;
        return reinterpret_cast<float*>(base + off);
    }
    void release(float* p, int level, bool force = false)
    {
        if (train && !force) return; // saved for backward
        freelist[level].push_back(reinterpret_cast<uintptr_t>(p) - base);
    }

    // packed-panel pointers (every mode's panels are PANEL_FLOATS * 4 bytes)
    const float* fwdp(long long off) const
    {
        return e->math ? reinterpret_cast<const float*>(e->pk_fwd_s) + off : e->pk_fwd + off;
    }
    const float* bwdp(long long off) const
    {
        return e->math ? reinterpret_cast<const float*>(e->pk_bwd_s) + off : e->pk_bwd + off;
    }
    Launch conv_launch(const ConvParams& p_in, bool bias_from_params, long long bias_off)
    {
        ConvParams p = p_in;
        {
            const int nst = p.n_out > 1 ? p.n_out : p.n_in;
            for (int i = 0; i < nst; ++i) if (!p.wstep[i]) p.wstep[i] = p.wpanel + (long long)i * PANEL_FLOATS;
        }
        xsd_engine* eng = e;
        const double px = (double)p.B * p.H * p.W;
        const double flop = 2.0 * 9 * 32 * 32 * p.n_in * p.n_out * px;
        const double bytes = 128.0 * (p.n_in + p.n_out) * px;
        std::vector<Launch> pre;     // math mode 4: reductions for input planes nobody has reported yet
        if (e->math == 4) {
            for (int i = 0; i < p.n_in; ++i) p.amax_in[i] = slot_of(p.in[i], p.H, p.W, pre);
            for (int j = 0; j < p.n_out; ++j) {   // this launch reports its own outputs
                OutDesc& o = p.out[j];
                // every view of the plane this launch writes loses its slot: a shuffled view (shuf_out) is one of four that
                // interleave over the whole high-resolution plane, so the range is the view's full extent, not its first byte
                invalidate_range(reinterpret_cast<uintptr_t>(o.p), (size_t)p.B * (size_t)o.bs * sizeof(float));
                o.amax = new_slot();
                amax_valid[ViewKey(reinterpret_cast<uintptr_t>(o.p), o.rs, o.ps)] = o.amax;
            }
        }
        return [eng, p, pre, bias_from_params, bias_off, flop, bytes](hipStream_t s) mutable {
            if (bias_from_params) p.bias = eng->params + bias_off;
            p.dbg = eng->dbg;
            p.ablate = eng->ablate;
            p.zero = eng->zero_page;
            for (auto& f : pre) { hipError_t err = f(s); if (err != hipSuccess) return err; }
            return prof_launch(eng, PK_CONV, flop, bytes, s, [&]() { return launch_conv_any(eng, p, s); });
        };
    }
    // wgrad + fixed-order reduce into the flat gradient vector
    void wgrad_launch(std::vector<Launch>& ops, int level, const std::vector<PlaneIn>& xs, const std::vector<PlaneIn>& gs,
                      const ConvW& cw, float scale, int j0 = 0, int n0 = 0, int plane = 0)
    {
        xsd_engine* eng = e;
        WgradParams wp = wgrad_base(level);
        wp.n_in = (int)xs.size(); wp.n_g = (int)gs.size(); wp.nparts = wgrad_nparts(e, wp.n_in, wp.n_g);
        for (size_t i = 0; i < xs.size(); ++i) wp.x[i] = xs[i];
        for (size_t i = 0; i < gs.size(); ++i) wp.g[i] = gs[i];
        std::vector<Launch> pre;     // math mode 4: reductions for planes nobody has reported yet
        if (e->math == 4) {
            for (size_t i = 0; i < xs.size(); ++i) wp.amax_x[i] = slot_of(xs[i], wp.H, wp.W, pre);
            for (size_t i = 0; i < gs.size(); ++i) wp.amax_g[i] = slot_of(gs[i], wp.H, wp.W, pre);
        }
        WgradReduceParams rp;
        memset(&rp, 0, sizeof(rp));
        rp.nparts = wp.nparts; rp.n_in = wp.n_in; rp.n_g = wp.n_g; rp.cin_total = cw.cin; rp.cout_total = cw.cout;
        rp.shuffle = cw.shuffle; rp.scale = scale; rp.j0 = j0; rp.n0 = n0; rp.plane = plane;
        const long long w_off = cw.w_off, b_off = cw.b_off;
        const double px = (double)wp.B * wp.H * wp.W;
        const double flop = 2.0 * 9 * 32 * 32 * wp.n_in * wp.n_g * px;
        const double bytes = 128.0 * (wp.n_in + wp.n_g) * px; // SURVEY 8(d) rule: every X plane and every G plane once (the kernel itself re-reads G once per X plane)
        ops.push_back([eng, wp, rp, pre, w_off, b_off, flop, bytes](hipStream_t s) mutable {
            for (auto& f : pre) { hipError_t perr = f(s); if (perr != hipSuccess) return perr; }
            wp.partial = eng->wg_partial; wp.bias_partial = eng->wg_bias_partial;
            rp.partial = eng->wg_partial; rp.bias_partial = eng->wg_bias_partial;
            rp.dw = eng->b_grads + w_off; rp.db = eng->b_grads + b_off;
            wp.zero = eng->zero_page; wp.ablate = eng->ablate; wp.dbg = eng->dbg;
            hipError_t err = prof_launch(eng, PK_WGRAD, flop, bytes, s, [&]() { return eng->math >= 3 ? launch_wgrad_split(eng->math, eng->ablate, wp, s) : launch_wgrad_mfma(wp, s); });
            if (err != hipSuccess) return err;
            return launch_wgrad_reduce(rp, s);
        });
    }

    // A dense block's FIFTEEN (X_j, G_n) pairs (conv n + 1 reads x_0 .. x_n: j <= n) as ONE pair-list launch of the f16x3 kernel:
    // 16 parts x 15 slots = 240 workgroups (+ a 17th part on the 16 spare CUs), the 15 of a part side by side on one XCD walking the same tiles, so that every X and
    // every G tile comes from HBM once and from that XCD's L2 for the other pairs (10 planes read instead of the 20 of five
    // launches per G).  The step runs at the package power cap and HBM traffic is a third of a launch's dynamic energy
    // (DESIGN.md 6.5): bytes are what there is to save; the 16 CUs the launch leaves idle draw next to nothing.
    // The part count, the pair list (conv-major) and the five reductions' fields: wgrad_block_fill above, shared with xsd_test_wgrad_block;
    // the caller falls back to one launch per G when block_parts_per_xcd is 0.
    void wgrad_block_launch(std::vector<Launch>& ops, const Tensor* const xpl[5], const Tensor* const Gp[6], const ConvW* cw, float gscale)
    {
        xsd_engine* eng = e;
        WgradBlock k;
        k.wp = wgrad_base(0);
        std::vector<Launch> pre;
        for (int i = 0; i < 5; ++i) {
            k.wp.x[i] = std_in((*xpl[i])[0], 0); k.wp.g[i] = std_in((*Gp[i + 1])[0], 0);      // g[n] = G_{n+1}, the gradient at conv n+1's output
            if (e->math == 4) {
                k.wp.amax_x[i] = slot_of(k.wp.x[i], k.wp.H, k.wp.W, pre);
                k.wp.amax_g[i] = slot_of(k.wp.g[i], k.wp.H, k.wp.W, pre);
            }
        }
        int cin[5], cout[5];
        std::vector<long long> wo(5), bo(5);
        for (int n = 0; n < 5; ++n) { cin[n] = cw[n].cin; cout[n] = cw[n].cout; wo[n] = cw[n].w_off; bo[n] = cw[n].b_off; }
        wgrad_block_fill(k, wgrad_block_nparts(e), cin, cout, gscale, e->wg_partial, e->wg_bias_partial);
        const double px = (double)k.wp.B * k.wp.H * k.wp.W;
        const double flop = 2.0 * 9 * 32 * 32 * 15 * px;
        const double bytes = 128.0 * 10 * px;      // SURVEY 8(d) rule: every X plane and every G plane once
        ops.push_back([eng, k, pre, wo, bo, flop, bytes](hipStream_t s) mutable {
            for (auto& f : pre) { hipError_t perr = f(s); if (perr != hipSuccess) return perr; }
            k.wp.zero = eng->zero_page; k.wp.ablate = eng->ablate; k.wp.dbg = eng->dbg;
            hipError_t err = prof_launch(eng, PK_WGRAD, flop, bytes, s, [&]() { return launch_wgrad_split(eng->math, eng->ablate, k.wp, s); });
            if (err != hipSuccess) return err;
            for (int n = 0; n < 5; ++n) { k.rp[n].dw = eng->b_grads + wo[n]; k.rp[n].db = eng->b_grads + bo[n]; }
            return wgrad_block_reduce(k, false, s);
        });
    }

    // ---------------------------------------------------------------------------------------------------------
    // The RRDB generator, once, for every configuration the plane kernels take: num_filters = 32 P (P = 1..8), 1..8 image channels
    // -- the shipped net is P = 1, the dense block's own default width is 64 (rrdb_blocks.py:23).  A feature tensor is P planes of
    // 32 channels in torch.cat's channel order; a conv with 32 a inputs and 32 b outputs is b output chunks, each ONE K-loop
    // over the a input planes, cut into launches of <= 5 planes: the first launch carries the bias, the later ones add to the
    // plane it wrote (`accumulate` epilogue), the last one carries the layer's epilogue (residuals, LeakyReLU, masks).  Packed
    // panels are in [chunk][plane] (forward) / [plane][chunk] (input gradient) order (pack_weights*_kernel).
    // The shipped configuration (`single`: one plane, one image channel each way) is this schedule plus five fast forms, each
    // marked `single` below with what it really needs: max |x| reported by edge_expand, compact LeakyReLU' mask words, the
    // diagnostic batch-chunk sweep, the dense block's pair-list weight-gradient launch, the shuffle conv as one 4-output launch.
    void build()
    {
        xsd_engine* eng = e;
        const int P = e->planes;
        const int blocks = e->cfg.num_res_blocks;
        const bool sr = e->cfg.kind == XSD_KIND_SR;
        const int nup = sr ? e->cfg.num_upsample : 0;
        std::vector<Launch>& F = e->fwd_ops;
        F.clear();
        e->bwd_stages.assign(blocks + 2, {});
        const int CI = e->cfg.in_channels, CO = e->cfg.out_channels;    // image channels: the image-side layers run one (image channel, plane) at a time
        const float* edge = e->pk_edge;      // [first_fwd | first_bwd][in channel][plane][288], [last_fwd | last_bwd][out channel][plane][288]
        auto first_fwd = [&](int ch, int q) { return edge + 288 * (ch * P + q); };
        auto first_bwd = [&](int ch, int q) { return edge + 288 * (P * CI + ch * P + q); };
        auto last_fwd = [&](int co, int q) { return edge + 288 * (2 * P * CI + co * P + q); };
        auto last_bwd = [&](int co, int q) { return edge + 288 * (2 * P * CI + P * CO + co * P + q); };
        const long long HW = (long long)H * W;
        const bool single = P == 1 && CI == 1 && CO == 1;

        auto alloc_t = [&](int level) { Tensor t(P); for (auto& p : t) p = alloc(level); return t; };
        auto release_t = [&](const Tensor& t, int level, bool force = false) { for (float* p : t) release(p, level, force); };
        auto planes_of = [&](const Tensor& t, int level) { std::vector<PlaneIn> v; for (float* p : t) v.push_back(std_in(p, level)); return v; };
        auto out_desc = [&](float* p, int level) { OutDesc o = conv_base(level).out[0]; std_out(o, p, level); return o; };
        // row `row` of a conv's packed panels `w`: the n consecutive panels of one K-loop
        auto panels = [&](const float* w, long long row, int n) { std::vector<const float*> v; for (int k = 0; k < n; ++k) v.push_back(w + (row * n + k) * PANEL_FLOATS); return v; };
        // one output plane: the K-loop over `ins` with the panels `pan` (one per input plane), <= 5 planes per launch
        // (nb > 0: restricted to the images [b0, b0 + nb))
        auto kloop = [&](std::vector<Launch>& ops, int level, const std::vector<PlaneIn>& ins, const std::vector<const float*>& pan,
                         const OutDesc& fin, bool bias_from_params, long long bias_off, const float* bias_ptr, int b0 = 0, int nb = 0) {
            const int n = (int)ins.size();
            for (int base = 0; base < n; base += 5) {
                const int cnt = std::min(5, n - base);
                const bool first = base == 0, last = base + cnt >= n;
                ConvParams p = conv_base(level);
                p.n_in = cnt; p.n_out = 1;
                for (int k = 0; k < cnt; ++k) { p.in[k] = ins[base + k]; p.wstep[k] = pan[base + k]; }
                p.wpanel = p.wstep[0];
                OutDesc& o = p.out[0];
                if (last) o = fin;
                else { o.p = fin.p; o.ps = fin.ps; o.rs = fin.rs; o.bs = fin.bs; o.a1 = fin.a1; }   // partial sums carry the final scale
                o.accumulate = first ? 0 : 1;
                if (first) p.bias = bias_ptr;
                ops.push_back(conv_launch(nb ? slice(p, b0, nb) : p, first && bias_from_params, bias_off));
            }
        };
        // weight gradient of one conv: per output chunk, the input planes in groups of <= 5
        auto wgrad_all = [&](std::vector<Launch>& ops, int level, const std::vector<PlaneIn>& xs, const Tensor& g, const ConvW& cw, float scale) {
            for (int q = 0; q < P; ++q)
                for (int base = 0; base < (int)xs.size(); base += 5) {
                    std::vector<PlaneIn> grp(xs.begin() + base, xs.begin() + std::min<size_t>(xs.size(), base + 5));
                    wgrad_launch(ops, level, grp, {std_in(g[q], level)}, cw, scale, base, q, 0);
                }
        };
        struct RdbAct { Tensor xin, xs[4], out; unsigned short* xb[4] = {}; };
        // compact lrelu' mask words of the dense blocks' activations (role-split conv epilogues) instead of the activation planes as masks.
        // `single`; needs P == 1: the epilogue that writes / reads the words has no `accumulate` variant, so the K-loop must be one launch
        const bool rdb_bits = single && train && e->math >= 3;
        std::vector<RdbAct> acts(blocks * 3);
        std::vector<Tensor> rin(blocks + 1);

        // ---- forward ------------------------------------------------------------------------------------------
        Tensor fea = alloc_t(0);
        for (int q = 0; q < P; ++q)   // conv_first (generator_rrdb.py:67), 32 output channels of one image channel per launch
            for (int ch = 0; ch < CI; ++ch) {
                EdgeExpandParams p; memset(&p, 0, sizeof(p));
                p.B = B; p.H = H; p.W = W; p.out = fea[q]; p.w = first_fwd(ch, q); p.mslope = 1.f; p.s_bs = CI * HW; p.accumulate = ch > 0;
                // `single`; needs CI == 1: the kernel reports the maximum of what it WRITES and so refuses `amax` with `accumulate`
                // (partial sums); elsewhere the first consumer sweeps the plane (plane_amax)
                if (single) p.amax = report_slot(fea[q], 0);
                const long long boff = e->first_b + 32 * q, xo = ch * HW;
                F.push_back([eng, p, boff, xo, ch](hipStream_t s) mutable {
                    p.s = eng->b_x + xo; p.bias = ch == 0 ? eng->params + boff : nullptr; return run_edge_expand(eng, p, s); });
            }
        Tensor cur = fea;
        for (int i = 0; i < blocks; ++i) {
            rin[i] = cur;
            for (int r = 0; r < 3; ++r) {
                RdbAct& a = acts[i * 3 + r];
                a.xin = cur;
                for (int c = 0; c < 5; ++c) {
                    (c < 4 ? a.xs[c] : a.out) = alloc_t(0);
                    if (c < 4 && rdb_bits) a.xb[c] = reinterpret_cast<unsigned short*>(alloc_img(0, 1));
                }
                // Diagnostic (e->chunk): sweep the dense block in batch chunks -- with <= 1-2 images per sweep the block's six planes
                // (6 x 33.5 MB per 512^2 image) stay in the Infinity Cache between conv_k and conv_{k+1..5}.
                // `single`; needs P == 1: slice() cuts single-launch convs only
                const int cb = (single && e->chunk > 0 && e->chunk < B) ? e->chunk : B;
                for (int b0 = 0; b0 < B; b0 += cb)
                    for (int c = 0; c < 5; ++c) {
                        const ConvW& cw = e->rdb[(i * 3 + r) * 5 + c];
                        const int ns = (c + 1) * P;
                        std::vector<PlaneIn> ins;
                        for (int t = 0; t <= c; ++t) for (float* pl : (t == 0 ? a.xin : a.xs[t - 1])) ins.push_back(std_in(pl, 0));
                        for (int q = 0; q < P; ++q) {
                            OutDesc fin = out_desc((c < 4 ? a.xs[c] : a.out)[q], 0);
                            if (c < 4) { fin.slope = 0.2f; fin.bits_out = a.xb[c]; }                       // rrdb_blocks.py:38-52
                            else {
                                fin.a1 = 0.2f; fin.e1 = a.xin[q]; fin.s1 = 1.f;                            // x5*0.2 + x   (:54)
                                if (r == 2) { fin.a2 = 0.2f; fin.e2 = rin[i][q]; fin.s2 = 1.f; }           // out*0.2 + x (:70)
                            }
                            kloop(F, 0, ins, panels(fwdp(cw.fwd_off), q, ns), fin, true, cw.b_off + 32 * q, nullptr, b0, std::min(cb, B - b0));
                        }
                    }
                for (int k = 0; k < 4; ++k) release_t(a.xs[k], 0);
                if (r > 0) release_t(a.xin, 0);
                cur = a.out;
            }
            if (i > 0) release_t(rin[i], 0);
        }
        rin[blocks] = cur;
        Tensor T = alloc_t(0);
        for (int q = 0; q < P; ++q) { // fea + trunk_conv(rrdb(fea)) (generator_rrdb.py:68-69)
            OutDesc fin = out_desc(T[q], 0);
            fin.e1 = fea[q]; fin.s1 = 1.f;
            kloop(F, 0, planes_of(cur, 0), panels(fwdp(e->trunk.fwd_off), q, P), fin, true, e->trunk.b_off + 32 * q, nullptr);
        }
        release_t(cur, 0);
        release_t(fea, 0);

        std::vector<Tensor> U(nup);
        Tensor H1;
        const int lo = nup; // output level
        if (sr) {
            Tensor feat = T;
            for (int u = 0; u < nup; ++u) { // upsampling: conv 32P -> 128P, LeakyReLU(0.01), PixelShuffle(2) (generator_rrdb.py:93-99)
                U[u] = alloc_t(u + 1);
                if (single) {   // the four sub-pixel chunks as ONE 4-output launch that publishes one maximum (alias_shuffled); needs P == 1: one input plane
                    ConvParams p = conv_base(u);
                    p.n_in = 1; p.n_out = 4; p.in[0] = std_in(feat[0], u); p.wpanel = fwdp(e->up[u].fwd_off);
                    for (int n = 0; n < 4; ++n) { shuf_out(p.out[n], U[u][0], u, n); p.out[n].slope = 0.01f; }
                    p.bias = e->pk_sbias + e->up[u].sbias_off;
                    F.push_back(conv_launch(p, false, 0));
                    alias_shuffled(U[u][0], u);
                }
                else for (int q = 0; q < P; ++q)
                    for (int sub = 0; sub < 4; ++sub) {           // chunk n = sub * P + q holds the channels 4 (32 q + c) + sub
                        const int n = sub * P + q;
                        OutDesc fin = conv_base(u).out[0];
                        shuf_out(fin, U[u][q], u, sub);
                        fin.slope = 0.01f;
                        kloop(F, u, planes_of(feat, u), panels(fwdp(e->up[u].fwd_off), n, P), fin, false, 0, e->pk_sbias + e->up[u].sbias_off + 32 * n);
                    }
                release_t(feat, u);
                feat = U[u];
            }
            H1 = alloc_t(lo);
            for (int q = 0; q < P; ++q) { // lrelu(HRconv(fea)) (generator_rrdb.py:107)
                OutDesc fin = out_desc(H1[q], lo);
                fin.slope = 0.2f;
                kloop(F, lo, planes_of(feat, lo), panels(fwdp(e->hr.fwd_off), q, P), fin, true, e->hr.b_off + 32 * q, nullptr);
            }
            release_t(feat, lo);
        }
        const long long HWo = (long long)(H << lo) * (W << lo);
        float* pre = train ? alloc_img(lo, CO) : nullptr;
        const Tensor& headf = sr ? H1 : T;
        // conv_last (+x for DN) + clamp, clamp (generator_rrdb.py:107-108,132-135; model.py:49): per output channel the planes' partial
        // sums chained in place through y, the last launch adds the skip and clamps
        for (int co = 0; co < CO; ++co)
            for (int q = 0; q < P; ++q) {
                EdgeReduceParams p; memset(&p, 0, sizeof(p));
                p.B = B; p.H = H << lo; p.W = W << lo; p.f = headf[q]; p.w = last_fwd(co, q); p.y_bs = CO * HWo; p.skip_bs = CI * HW;
                const bool first = q == 0, last = q == P - 1;
                const long long boff = e->last_b + co, yo = co * HWo, xo = (CI == 1 ? 0 : co) * HW;   // DN: x broadcasts when it has one channel
                F.push_back([eng, p, first, last, boff, yo, xo, pre, sr](hipStream_t s) mutable {
                    p.y = eng->b_y + yo;
                    if (first) p.bias = eng->params + boff; else p.addto = p.y;
                    if (last) { p.skip = sr ? nullptr : eng->b_x + xo; p.pre = pre ? pre + yo : nullptr; p.clamp01 = 1; }
                    return run_edge_reduce(eng, p, s);
                });
            }
        if (!train) return;

        // ---- backward -----------------------------------------------------------------------------------------
        e->amax_bwd_first = e->amax_used;      // every slot from here on is first written by a backward launch
        float* dpre = alloc_img(lo, CO);
        Tensor dT = alloc_t(0);
        { // stage 0: output head
            std::vector<Launch>& S = e->bwd_stages[0];
            const long long npx = (long long)B * CO * HWo;
            S.push_back([eng, pre, dpre, npx](hipStream_t s) { return prof_launch(eng, PK_CLAMP_BWD, 0.0, 12.0 * npx, s, [&]() { return launch_clamp_bwd(pre, eng->b_dy, dpre, npx, s); }); });
            for (int co = 0; co < CO; ++co)
            for (int q = 0; q < P; ++q) { // conv_last weight grad, 32 input channels of one output channel per launch (the bias gradient is the same sum every time)
                EdgeWgradParams p; memset(&p, 0, sizeof(p));
                p.B = B; p.H = H << lo; p.W = W << lo; p.f = headf[q]; p.s = dpre + co * HWo; p.s_bs = CO * HWo; p.nblocks = edge_wgrad_nblocks();
                const long long wo = e->last_w + ((long long)co * 32 * P + 32 * q) * 9, bo = e->last_b + co;
                S.push_back([eng, p, wo, bo](hipStream_t s) mutable {
                    p.partial = eng->edge_partial; return run_edge_wgrad(eng, p, 1, eng->b_grads + wo, eng->b_grads + bo, s);
                });
            }
            Tensor GH = sr ? alloc_t(lo) : dT;      // conv_last's input gradient: DN d(T); SR d(H1) masked by lrelu'(0.2)
            for (int q = 0; q < P; ++q)   // the output channels' contributions summed, the mask on the last
                for (int co = 0; co < CO; ++co) {
                    EdgeExpandParams p; memset(&p, 0, sizeof(p));
                    p.B = B; p.H = H << lo; p.W = W << lo; p.s = dpre + co * HWo; p.s_bs = CO * HWo; p.w = last_bwd(co, q); p.out = GH[q];
                    p.accumulate = co > 0; p.mslope = 1.f;
                    if (sr && co == CO - 1) { p.mask = H1[q]; p.mslope = 0.2f; }
                    if (single) p.amax = report_slot(GH[q], lo);      // needs CO == 1: no `amax` with `accumulate`, as on conv_first
                    S.push_back([eng, p](hipStream_t s) { return run_edge_expand(eng, p, s); });
                }
            if (sr) {
                const Tensor& hr_in = nup > 0 ? U[nup - 1] : T;
                wgrad_all(S, lo, planes_of(hr_in, lo), GH, e->hr, 1.f);
                Tensor G = nup > 0 ? alloc_t(lo) : dT;
                for (int pl = 0; pl < P; ++pl) { // HRconv input gradient (masked by the upsample LeakyReLU(0.01) when it feeds a pixel-shuffle)
                    OutDesc fin = out_desc(G[pl], lo);
                    if (nup > 0) { fin.mask = U[nup - 1][pl]; fin.mslope = 0.01f; }
                    kloop(S, lo, planes_of(GH, lo), panels(bwdp(e->hr.bwd_off), pl, P), fin, false, 0, nullptr);
                }
                for (int u = nup - 1; u >= 0; --u) {
                    const Tensor& xin = u > 0 ? U[u - 1] : T;
                    for (int q = 0; q < P; ++q) {                 // dW of the shuffle conv: the four sub-pixel views of gradient plane q against every input plane
                        std::vector<PlaneIn> gs;
                        for (int sub = 0; sub < 4; ++sub) gs.push_back(shuf_in(G[q], u, sub));
                        for (int j = 0; j < P; ++j) wgrad_launch(S, u, {std_in(xin[j], u)}, gs, e->up[u], 1.f, j, 0, q);
                    }
                    Tensor Gn = u > 0 ? alloc_t(u) : dT;
                    for (int pl = 0; pl < P; ++pl) {
                        std::vector<PlaneIn> ins;      // chunk sub * P + q of the shuffle conv's output, in panel order
                        for (int sub = 0; sub < 4; ++sub)
                            for (int q = 0; q < P; ++q) ins.push_back(shuf_in(G[q], u, sub));
                        OutDesc fin = out_desc(Gn[pl], u);
                        if (u > 0) { fin.mask = U[u - 1][pl]; fin.mslope = 0.01f; }
                        kloop(S, u, ins, panels(bwdp(e->up[u].bwd_off), pl, 4 * P), fin, false, 0, nullptr);
                    }
                    G = Gn;
                }
            }
            // trunk_conv
            wgrad_all(S, 0, planes_of(rin[blocks], 0), dT, e->trunk, 1.f);
        }
        Tensor dR = alloc_t(0);
        for (int pl = 0; pl < P; ++pl)
            kloop(e->bwd_stages[0], 0, planes_of(dT, 0), panels(bwdp(e->trunk.bwd_off), pl, P), out_desc(dR[pl], 0), false, 0, nullptr);
        Tensor dS[5] = {Tensor(), alloc_t(0), alloc_t(0), alloc_t(0), alloc_t(0)};
        for (int i = blocks - 1; i >= 0; --i) {
            std::vector<Launch>& S = e->bwd_stages[blocks - i];
            Tensor dOut = dR;
            for (int r = 2; r >= 0; --r) {
                const RdbAct& a = acts[i * 3 + r];
                const float gscale = r == 2 ? 0.04f : 0.2f;
                const ConvW* cw = &e->rdb[(i * 3 + r) * 5];
                dS[0] = alloc_t(0);
                const Tensor* xpl[5] = {&a.xin, &a.xs[0], &a.xs[1], &a.xs[2], &a.xs[3]};
                // Input-gradients as K-loops (no read-modify-write): dS_j = sum_{c>j} conv^T_c[j](G_c) in ONE K-loop over
                // the planes of G_5 = dOut, G_4..G_{j+1}; its epilogue adds the residual-path terms (j = 0) or applies
                // lrelu'(x_j) (j >= 1), which makes dS_j the G_j of conv_j.  conv5's 0.2 / 0.04 factor lives in its
                // transposed panels (PackDesc.bwd_scale); its weight gradient uses the unscaled dOut and scales in the reduce.
                const Tensor* Gp[6] = {nullptr, &dS[1], &dS[2], &dS[3], &dS[4], &dOut}; // G_c, c = 1..5
                // one pair-list weight-gradient launch per dense block (f16x3 kernel) once every G exists, i.e. in front of dS_0
                // (XSD_WGRAD_BLOCK=0 restores one launch per G for same-library A/Bs: 122.6 -> 125.6 tiles/s on one device, profiles/r04_ab_wgrad_block_launch.txt)
#ifdef XSD_TEST_HOOKS
                static const bool block_wgrad = getenv("XSD_WGRAD_BLOCK") ? atoi(getenv("XSD_WGRAD_BLOCK")) != 0 : true;
#else
                constexpr bool block_wgrad = true;
#endif
                // `single`; needs P == 1: the pair list is the fifteen (X, G) pairs of one-plane tensors.  Both role-split weight-gradient
                // kernels take pair lists; fewer than 120 CUs: one launch per G
                const bool mega = single && block_wgrad && e->math >= 3 && block_parts_per_xcd(e->ncu) >= 1;
                for (int c = 4; c >= 0; --c) { // conv index c (0-based) = conv_{c+1}
                    std::vector<PlaneIn> xs;
                    for (int t = 0; t <= c; ++t) for (float* pl : *xpl[t]) xs.push_back(std_in(pl, 0));
                    if (!mega) wgrad_all(S, 0, xs, *Gp[c + 1], cw[c], c == 4 ? gscale : 1.f);
                    else if (c == 0) wgrad_block_launch(S, xpl, Gp, cw, gscale);
                    // now every G needed by dS_c exists: G_5 .. G_{c+1}
                    const int j = c;
                    for (int pl = 0; pl < P; ++pl) {
                        std::vector<PlaneIn> ins;
                        std::vector<const float*> pan;
                        for (int ii = 0; ii < 5 - j; ++ii) {
                            const int cc = 5 - ii;          // 1-based conv whose gradient planes these are; its input plane index of (tensor j, plane pl) is j P + pl
                            for (int q = 0; q < P; ++q) {
                                ins.push_back(std_in((*Gp[cc])[q], 0));
                                pan.push_back(bwdp(cw[cc - 1].bwd_off + (((long long)j * P + pl) * P + q) * PANEL_FLOATS));
                            }
                        }
                        OutDesc fin = out_desc(dS[j][pl], 0);
                        if (j == 0) {
                            fin.e1 = dOut[pl]; fin.s1 = r == 2 ? 0.2f : 1.f;
                            if (r == 0) { fin.e2 = dR[pl]; fin.s2 = 1.f; if (i == 0) { fin.e3 = dT[pl]; fin.s3 = 1.f; } }
                        } else { fin.mask = (*xpl[j])[pl]; fin.mslope = 0.2f; fin.bits_in = a.xb[j - 1]; }
                        kloop(S, 0, ins, pan, fin, false, 0, nullptr);
                    }
                }
                if (dOut[0] != dR[0]) release_t(dOut, 0, true);
                dOut = dS[0];
            }
            release_t(dR, 0, true);
            dR = dOut;
        }
        { // last stage: conv_first weight grad and (optionally) dx
            std::vector<Launch>& S = e->bwd_stages[blocks + 1];
            const Tensor dFea = dR;
            for (int ch = 0; ch < CI; ++ch)
                for (int q = 0; q < P; ++q) {
                    EdgeWgradParams p; memset(&p, 0, sizeof(p));
                    p.B = B; p.H = H; p.W = W; p.f = dFea[q]; p.nblocks = edge_wgrad_nblocks(); p.s_bs = CI * HW;
                    const long long wo = e->first_w + ((long long)32 * q * CI + ch) * 9, bo = e->first_b + 32 * q, xo = ch * HW;
                    const int cstride = 9 * CI;
                    S.push_back([eng, p, wo, bo, xo, cstride](hipStream_t s) mutable {
                        p.s = eng->b_x + xo; p.partial = eng->edge_partial;
                        return run_edge_wgrad(eng, p, 0, eng->b_grads + wo, eng->b_grads + bo, s, cstride);
                    });
                }
            const bool bcast = !sr && CI == 1 && CO > 1;  // DN with a one-channel x added to every output channel: dx += sum over the channels of dpre
            const float* skipg = (sr || bcast) ? nullptr : dpre;     // DN: d(out + x)/dx per channel
            // dx per image channel: the planes' partial sums chained in place (all launches skipped when the caller wants no dx)
            for (int ch = 0; ch < CI; ++ch)
                for (int q = 0; q < P; ++q) {
                    EdgeReduceParams p; memset(&p, 0, sizeof(p));
                    p.B = B; p.H = H; p.W = W; p.f = dFea[q]; p.w = first_bwd(ch, q); p.y_bs = CI * HW; p.skip_bs = CO * HW;
                    const bool first = q == 0, last = q == P - 1;
                    const long long xo = ch * HW;
                    S.push_back([eng, p, first, last, xo, skipg](hipStream_t s) mutable {
                        if (!eng->b_dx) return hipSuccess;
                        p.y = eng->b_dx + xo;
                        if (!first) p.addto = p.y;
                        if (last && skipg) p.skip = skipg + xo;
                        return run_edge_reduce(eng, p, s);
                    });
                }
            if (bcast) {
                const int nb = B, nc = CO;
                S.push_back([eng, dpre, nb, nc, HW](hipStream_t s) { return eng->b_dx ? launch_add_channels(eng->b_dx, dpre, nc, HW, nb, s) : hipSuccess; });
            }
        }
    }
};

static int ensure_plan(xsd_engine* e, int B, int H, int W, bool train)
{
    if (e->pB == B && e->pH == H && e->pW == W && e->ptrain == (int)train) return XSD_OK;
    e->pB = e->pH = e->pW = 0; e->ptrain = -1; e->fwd_saved = false;
    Builder sizing(e, B, H, W, train, 0);
    e->amax_used = 2;
    sizing.build();
    const size_t need = sizing.peak + 256;
    if (need > e->ws_bytes) {
        // A batch that cannot fit is refused BEFORE the workspace the engine holds is given up: what the device could offer at best is
        // its free memory plus that workspace.  The engine stays usable (same plan cache state as after any other shape change), and
        // the message names the way out the reference has for this (rrdb_blocks.py:39-47: recompute instead of keeping activations).
        const double gb = 1.0 / (1024.0 * 1024.0 * 1024.0);
        const char* hint = train ? "; the saved activations of a training step are ~7.9 KB per low-resolution pixel -- construct the generator with "
                                   "memory_efficient=True (chunked recompute, XSD_ME_CHUNK tiles at a time: the reference's rrdb_blocks.py:39-47 policy) or use a smaller batch"
                                 : "; use a smaller batch per call";
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need > free_b + e->ws_bytes)
            return fail(XSD_ERR_NOMEM, "a workspace of %.1f GiB for %d x %d x %d tiles does not fit this device (%.1f GiB free + %.1f GiB held by this engine of %.1f GiB)%s",
                        need * gb, B, H, W, free_b * gb, e->ws_bytes * gb, total_b * gb, hint);
        if (e->ws) { hipDeviceSynchronize(); xsd::dev_free(e->ws); e->ws = nullptr; e->ws_bytes = 0; }
        hipError_t err = xsd::dev_alloc((void**)&e->ws, need);
        if (err != hipSuccess) {
            (void)hipGetLastError();      // the failed allocation must not surface again as the next launch's error
            return fail(XSD_ERR_NOMEM, "workspace allocation (%.1f GiB for %d x %d x %d tiles) failed: %s%s", need * gb, B, H, W, hipGetErrorString(err), hint);
        }
        e->ws_bytes = need;
    }
    if (e->amax_used + xsd_engine::AMAX_TAIL > e->amax_cap) {     // the sizing pass counted more max-|x| slots than are allocated
        const int cap = ((e->amax_used + xsd_engine::AMAX_TAIL + 4095) / 4096) * 4096;
        hipDeviceSynchronize();
        float* grown = nullptr;
        hipError_t err = xsd::dev_alloc((void**)&grown, sizeof(float) * (size_t)cap);
        if (err == hipSuccess) err = hipMemset(grown, 0, sizeof(float) * (size_t)cap);
        if (err != hipSuccess) { if (grown) xsd::dev_free(grown); return fail(XSD_ERR_NOMEM, "max-|x| slot array allocation (%d floats) failed: %s", cap, hipGetErrorString(err)); }
        if (e->amax) {      // slots 0 / 1 hold the packed panels' maxima (written by the last xsd_pack_weights): they move along
            err = hipMemcpy(grown, e->amax, 2 * sizeof(float), hipMemcpyDeviceToDevice);
            if (err != hipSuccess) { xsd::dev_free(grown); return fail(XSD_ERR_HIP, "max-|x| slot copy failed: %s", hipGetErrorString(err)); }
            xsd::dev_free(e->amax);
        }
        // hipMemset / hipMemcpy above run on stream 0, the launches that read the slots on the caller's stream, which may be non-blocking
        // (no implicit order with stream 0); neither call is documented to have completed on the device when it returns (a memset of
        // device memory may be asynchronous to the host; hipFree's implicit device synchronize runs only when there was an old array)
        err = hipDeviceSynchronize();
        if (err != hipSuccess) { xsd::dev_free(grown); e->amax = nullptr; e->amax_cap = 0; return fail(XSD_ERR_HIP, "max-|x| slot array: %s", hipGetErrorString(err)); }
        e->amax = grown; e->amax_cap = cap;
    }
    e->amax_used = 2;
    e->amax_bwd_first = 1 << 30;      // a forward-only plan has no backward slots; build() sets it where the backward stages begin
    Builder real(e, B, H, W, train, reinterpret_cast<uintptr_t>(e->ws));
    real.build();
    e->pB = B; e->pH = H; e->pW = W; e->ptrain = (int)train;
    return XSD_OK;
}

// ------------------------------------------------------------------------------------------------------------
// zero-padded widths: expansion of the caller's parameters / gathering of the gradients
// ------------------------------------------------------------------------------------------------------------
__global__ void pad_params_kernel(const float* real, float* padded, const PadDesc* descs, int to_real /* 0: expand params, 1: gather grads */)
{
    const PadDesc d = descs[blockIdx.y];
    const long long nw = (long long)d.cout_r * d.cin_r * 9;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < nw + d.cout_r; e += (long long)gridDim.x * blockDim.x) {
        long long r, q;
        if (e < nw) {
            const int tap = (int)(e % 9), ic = (int)((e / 9) % d.cin_r), oc = (int)(e / (9ll * d.cin_r));
            const int icp = (ic / d.tin_r) * d.tin_p + ic % d.tin_r;
            r = d.w_r + e; q = d.w_p + ((long long)oc * d.cin_p + icp) * 9 + tap;
        } else { r = d.b_r + (e - nw); q = d.b_p + (e - nw); }
        if (to_real) const_cast<float*>(real)[r] = padded[q]; else padded[q] = real[r];
    }
}
hipError_t launch_pad_params(const float* real, float* padded, const PadDesc* descs_dev, int ndesc, int to_real, hipStream_t s)
{
    hipLaunchKernelGGL(pad_params_kernel, dim3(64, ndesc), dim3(256), 0, s, real, padded, descs_dev, to_real);
    return hipGetLastError();
}

// OIHW weights -> packed panels of math mode `math`, for the `ndesc` convs of a descriptor table: xsd_pack_weights with the engine's
// buffers, the test entries' single-conv packer with its temporaries.  Mode 0 fills pk_fwd / pk_bwd, mode 3 pk_fwd_s / pk_bwd_s, mode 4
// all four and the two max-|w| slots amax2[0] (forward panels), amax2[1] (input-gradient panels).
hipError_t pack_panels(int math, const float* dev_params, const PackDesc* descs_dev, int ndesc, float* pk_fwd, float* pk_bwd,
                       void* pk_fwd_s, void* pk_bwd_s, long long pk_floats, float* amax2, hipStream_t s)
{
    if (math == 3) return launch_pack_weights_s3(dev_params, descs_dev, ndesc, static_cast<float*>(pk_fwd_s), static_cast<float*>(pk_bwd_s), s);
    if (math != 4) return launch_pack_weights(dev_params, descs_dev, ndesc, pk_fwd, pk_bwd, s);
    // fp32 fragment-order panels into the (otherwise unused) mode-0 buffers, max |w| of the forward and of the
    // input-gradient panels (one power-of-two scale each), then the two-term fp16 images the conv kernel copies to LDS
    hipError_t err = launch_pack_weights_s3(dev_params, descs_dev, ndesc, pk_fwd, pk_bwd, s);
    if (err == hipSuccess) err = hipMemsetAsync(amax2, 0, 2 * sizeof(float), s);
    if (err == hipSuccess) err = launch_buffer_amax(pk_fwd, pk_floats, amax2 + 0, s);
    if (err == hipSuccess) err = launch_buffer_amax(pk_bwd, pk_floats, amax2 + 1, s);
    if (err == hipSuccess) err = launch_split_panels_f16(pk_fwd, pk_fwd_s, pk_floats, amax2 + 0, s);
    if (err == hipSuccess) err = launch_split_panels_f16(pk_bwd, pk_bwd_s, pk_floats, amax2 + 1, s);
    return err;
}

// ------------------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------------------
extern "C" {

const char* xsd_last_error(void) { return g_err.c_str(); }
#if defined(XSD_DIAG)
const char* xsd_version(void) { return "xsd-hip gfx950 r6 (diagnostic variant)"; }
#elif defined(XSD_TEST_HOOKS)
const char* xsd_version(void) { return "xsd-hip gfx950 r6 (test-hooks variant)"; }
#else
const char* xsd_version(void) { return "xsd-hip gfx950 r6"; }
#endif

int xsd_create(const xsd_config* cfg, xsd_engine** out)
{
    if (!cfg || !out) return fail(XSD_ERR_ARG, "null argument");
    if (cfg->kind != XSD_KIND_DN && cfg->kind != XSD_KIND_SR) return fail(XSD_ERR_ARG, "kind must be 0 (DN) or 1 (SR)");
    if (cfg->in_channels < 1 || cfg->out_channels < 1 || cfg->num_filters < 1 || cfg->in_channels > 1024 || cfg->out_channels > 1024 || cfg->num_filters > 1024)
        return fail(XSD_ERR_ARG, "in_channels, out_channels and num_filters must be in [1,1024] (got %d,%d,%d)", cfg->in_channels, cfg->out_channels, cfg->num_filters);
    // GeneratorRRDB_DN adds its input to the conv_last output (generator_rrdb.py:134): the shapes must broadcast
    if (cfg->kind == XSD_KIND_DN && cfg->in_channels != cfg->out_channels && cfg->in_channels != 1)
        return fail(XSD_ERR_ARG, "DN: `out + x` needs in_channels == out_channels or in_channels == 1 (got %d,%d)", cfg->in_channels, cfg->out_channels);
    if (cfg->num_res_blocks < 1 || cfg->num_res_blocks > 64) return fail(XSD_ERR_ARG, "num_res_blocks must be in [1,64]");
    if (cfg->kind == XSD_KIND_SR && (cfg->num_upsample < 1 || cfg->num_upsample > 2)) return fail(XSD_ERR_ARG, "num_upsample must be 1 or 2");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(XSD_ERR_HIP, "no HIP device available");
    xsd_engine* e = new xsd_engine();
    e->cfg = *cfg;
    {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) e->ncu = prop.multiProcessorCount;
#ifdef XSD_TEST_HOOKS
        // test hooks (include/xsd.h; hooks variant only): plan as if the device had this many CUs; start the max-|x| slot array this small
        if (const char* m = getenv("XSD_TEST_NCU")) { const int v = atoi(m); if (v >= 8 && v <= 4096) e->ncu = v; }
        if (const char* m = getenv("XSD_TEST_AMAX_CAP")) { const int v = atoi(m); if (v >= 2 * xsd_engine::AMAX_TAIL && v <= e->amax_cap) e->amax_cap = v; }
#endif
    }
    // 32-channel planes (widths that are no multiple of 32 zero-padded to the next one), a few image channels
    const bool plane_path = cfg->num_filters <= 256 && cfg->in_channels <= 8 && cfg->out_channels <= 8 &&
                            (cfg->kind == XSD_KIND_SR || cfg->in_channels == cfg->out_channels || cfg->in_channels == 1);
    if (!plane_path) {
        // more than 256 filters or more than 8 image channels: the generic-width path (exact fp32)
        e->generic = GenericNet::create(*cfg);
        if (!e->generic) { delete e; return fail(XSD_ERR_NOMEM, "generic-width engine: device allocation failed"); }
        e->nparams = e->generic->nparams;
        if (xsd::dev_alloc((void**)&e->loss_partial, sizeof(double) * 1024) != hipSuccess) { xsd_destroy(e); return fail(XSD_ERR_NOMEM, "device allocation failed"); }
        *out = e;
        return XSD_OK;
    }
#ifdef XSD_DIAG   // the diagnostic library variant (make diag, selected with XSD_LIB) is the only build that reads these
    if (const char* m = getenv("XSD_ABLATE")) e->ablate = atoi(m);
    if (const char* m = getenv("XSD_CHUNK")) e->chunk = atoi(m);
#endif
    if (const char* m = getenv("XSD_MATH")) {
        if (strcmp(m, "f16x3") == 0 || strcmp(m, "4") == 0) e->math = 4;
        else if (strcmp(m, "bf16x6") == 0 || strcmp(m, "3") == 0) e->math = 3;
        else if (strcmp(m, "fp32") == 0 || strcmp(m, "0") == 0) e->math = 0;
        else { delete e; return fail(XSD_ERR_ARG, "XSD_MATH=%s: the math modes are fp32, bf16x6 and f16x3", m); }
    }
    const int blocks = cfg->num_res_blocks, nup = cfg->kind == XSD_KIND_SR ? cfg->num_upsample : 0;
    const int nf_r = cfg->num_filters, nf = (nf_r + 31) / 32 * 32;      // real / padded width
    const int CIc = cfg->in_channels, COc = cfg->out_channels;
    e->planes = nf / 32;
    if (nf != nf_r) e->nf_pad = nf;
    long long off = 0, pk = 0, sb = 0, off_r = 0;
    std::vector<PadDesc> pads;      // every conv in parameter order, with its place in the caller's (real-width) flat vector
    auto pad_add = [&](long long w_p, long long b_p, int cout_r, int cin_r, int cin_p, int tin_r, int tin_p) {
        PadDesc d; d.w_p = w_p; d.b_p = b_p; d.w_r = off_r; off_r += (long long)cout_r * cin_r * 9; d.b_r = off_r; off_r += cout_r;
        d.cout_r = cout_r; d.cin_r = cin_r; d.cin_p = cin_p; d.tin_r = tin_r; d.tin_p = tin_p;
        pads.push_back(d);
    };
    take_conv(off, nf, CIc, e->first_w, e->first_b);
    pad_add(e->first_w, e->first_b, nf_r, CIc, CIc, CIc, CIc);
    auto mk = [&](int cout, int cin, int shuffle) {
        ConvW c; take_conv(off, cout, cin, c.w_off, c.b_off);
        c.cout = cout; c.cin = cin; c.shuffle = shuffle;
        c.fwd_off = pk; c.bwd_off = pk; pk += (long long)(cout / 32) * (cin / 32) * PANEL_FLOATS;
        c.sbias_off = -1;
        if (shuffle) { c.sbias_off = sb; sb += cout; }
        pad_add(c.w_off, c.b_off, cout / nf * nf_r, cin / nf * nf_r, cin, nf_r, nf);      // cout, cin are multiples of the (padded) width
        return c;
    };
    for (int i = 0; i < blocks; ++i) {
        e->rrdb_begin.push_back(off);
        e->rrdb_begin_real.push_back(off_r);
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 5; ++c) {
                e->rdb.push_back(mk(nf, nf * (c + 1), 0));
                // conv5's gradient arrives as 0.2*dOut (x5*0.2 + x) and, for RDB3, 0.2*0.2*dOut (out*0.2 + x): fold it
                if (c == 4) e->rdb.back().bwd_scale = r == 2 ? 0.04f : 0.2f;
            }
    }
    e->rrdb_begin.push_back(off);
    e->rrdb_begin_real.push_back(off_r);
    e->trunk = mk(nf, nf, 0);
    take_conv(off, COc, nf, e->last_w, e->last_b);
    pad_add(e->last_w, e->last_b, COc, nf_r, nf, nf_r, nf);
    for (int u = 0; u < nup; ++u) e->up.push_back(mk(4 * nf, nf, 1));
    if (cfg->kind == XSD_KIND_SR) e->hr = mk(nf, nf, 0);
    e->nparams_pad = off;
    e->nparams_real = off_r;
    e->npad = (int)pads.size();
    e->nparams = e->nf_pad ? off_r : off;       // what the caller's flat vectors hold
    e->pk_floats = pk;

    std::vector<PackDesc> descs;
    auto add = [&](const ConvW& c) { PackDesc d; d.src_w = c.w_off; d.dst_fwd = c.fwd_off; d.dst_bwd = c.bwd_off; d.cout = c.cout; d.cin = c.cin; d.shuffle = c.shuffle; d.bwd_scale = c.bwd_scale; descs.push_back(d); };
    for (auto& c : e->rdb) add(c);
    add(e->trunk);
    for (auto& c : e->up) add(c);
    if (cfg->kind == XSD_KIND_SR) add(e->hr);
    e->ndesc = (int)descs.size();
#define CK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { int rc = fail(_e == hipErrorOutOfMemory ? XSD_ERR_NOMEM : XSD_ERR_HIP, "%s: %s", #expr, hipGetErrorString(_e)); xsd_destroy(e); return rc; } } while (0)
    CK(xsd::dev_alloc((void**)&e->pk_fwd, sizeof(float) * pk));
    CK(xsd::dev_alloc((void**)&e->pk_bwd, sizeof(float) * pk));
    CK(xsd::dev_alloc((void**)&e->pk_fwd_s, sizeof(float) * pk));
    CK(xsd::dev_alloc((void**)&e->pk_bwd_s, sizeof(float) * pk));
    if (e->nf_pad) {
        CK(xsd::dev_alloc((void**)&e->params_pad, sizeof(float) * e->nparams_pad));
        CK(xsd::dev_alloc((void**)&e->grads_pad, sizeof(float) * e->nparams_pad));
        CK(xsd::dev_alloc((void**)&e->pad_descs, sizeof(PadDesc) * pads.size()));
        CK(hipMemcpy(e->pad_descs, pads.data(), sizeof(PadDesc) * pads.size(), hipMemcpyHostToDevice));
    }
    CK(xsd::dev_alloc((void**)&e->amax, sizeof(float) * e->amax_cap));
    CK(hipMemset(e->amax, 0, sizeof(float) * e->amax_cap));
    CK(xsd::dev_alloc((void**)&e->zero_page, 512));   // [0,256): zeros (padding source); [256,512): trash (stores of lanes outside the image)
    CK(hipMemset(e->zero_page, 0, 512));
    CK(xsd::dev_alloc((void**)&e->pk_edge, sizeof(float) * 2 * 288 * e->planes * (cfg->in_channels + cfg->out_channels)));   // [first_fwd | first_bwd][in channel][plane][288], [last_fwd | last_bwd][out channel][plane][288]
    CK(xsd::dev_alloc((void**)&e->pk_sbias, sizeof(float) * (sb ? sb : 1)));
    CK(xsd::dev_alloc((void**)&e->descs_dev, sizeof(PackDesc) * descs.size()));
    CK(hipMemcpy(e->descs_dev, descs.data(), sizeof(PackDesc) * descs.size(), hipMemcpyHostToDevice));
    CK(xsd::dev_alloc((void**)&e->wg_partial, sizeof(float) * (size_t)e->nparts * 5 * PANEL_FLOATS));
    CK(xsd::dev_alloc((void**)&e->wg_bias_partial, sizeof(float) * (size_t)e->nparts * 4 * 32));
    CK(xsd::dev_alloc((void**)&e->edge_partial, sizeof(float) * EDGE_WGRAD_BLOCKS * 321));
    CK(xsd::dev_alloc((void**)&e->loss_partial, sizeof(double) * 1024));
    // the hipMemset / hipMemcpy above went to stream 0; the first pack and forward may come on a non-blocking stream, which stream 0 does
    // not order: what they read (zeroed slots, the zero page, the descriptors) is on the device before create returns
    CK(hipDeviceSynchronize());
#undef CK
    *out = e;
    return XSD_OK;
}

void xsd_destroy(xsd_engine* e)
{
    if (!e) return;
    hipDeviceSynchronize();
    delete e->generic;
    for (auto ev : e->ev_pool) hipEventDestroy(ev);
    xsd::dev_free(e->pk_fwd); xsd::dev_free(e->pk_bwd); xsd::dev_free(e->pk_fwd_s); xsd::dev_free(e->pk_bwd_s); xsd::dev_free(e->zero_page); xsd::dev_free(e->amax); xsd::dev_free(e->pk_edge); xsd::dev_free(e->pk_sbias); xsd::dev_free(e->descs_dev);
    xsd::dev_free(e->wg_partial); xsd::dev_free(e->wg_bias_partial); xsd::dev_free(e->edge_partial); xsd::dev_free(e->loss_partial);
    xsd::dev_free(e->ws); xsd::dev_free(e->params_pad); xsd::dev_free(e->grads_pad); xsd::dev_free(e->pad_descs);
    xsd::dev_free(e->dbg);       // held while xsd_debug_stamps is on
    delete e;
}

int64_t xsd_param_count(const xsd_engine* e) { return e ? e->nparams : 0; }

int xsd_set_math(xsd_engine* e, int mode)
{
    if (!e || (mode != 0 && mode != 3 && mode != 4)) return fail(XSD_ERR_ARG, "math mode must be 0 (fp32, exact), 3 (bf16x6) or 4 (f16x3); modes 1 and 2 (16-bit significands) were removed in round 3");
    if (e->generic) { e->math = mode; return XSD_OK; }   // the generic-width kernels are exact fp32 whatever the mode says
    if (mode != e->math) { e->math = mode; e->packed = false; e->pB = 0; e->ptrain = -1; e->fwd_saved = false; }
    return XSD_OK;
}
// what the kernels actually compute in: the exact-fp32 kernels of generic_net.hip serve every mode setting
int xsd_get_math(const xsd_engine* e) { return e ? (e->generic ? 0 : e->math) : -1; }

int xsd_pack_weights(xsd_engine* e, const float* dev_params, void* stream)
{
    if (!e || !dev_params) return fail(XSD_ERR_ARG, "null argument");
    hipStream_t s = (hipStream_t)stream;
    e->params = dev_params;
    if (e->generic) { HIPCHK(e->generic->pack(dev_params, s)); e->packed = true; return XSD_OK; }
    if (e->nf_pad) {     // the engine runs on the zero-padded copy
        HIPCHK(hipMemsetAsync(e->params_pad, 0, sizeof(float) * e->nparams_pad, s));
        HIPCHK(launch_pad_params(dev_params, e->params_pad, static_cast<const PadDesc*>(e->pad_descs), e->npad, 0, s));
        dev_params = e->params_pad;
        e->params = dev_params;
    }
    HIPCHK(pack_panels(e->math, dev_params, e->descs_dev, e->ndesc, e->pk_fwd, e->pk_bwd, e->pk_fwd_s, e->pk_bwd_s, e->pk_floats, e->amax, s));
    {   // conv_first W[c][ch][tap] and conv_last W[co][c][tap], 32 feature channels (one plane) of one image channel at a time
        const int P = e->planes, ci = e->cfg.in_channels, co = e->cfg.out_channels, nf = 32 * P;
        float* ff = e->pk_edge; float* fb = ff + 288 * P * ci; float* lf = fb + 288 * P * ci; float* lb = lf + 288 * P * co;
        for (int ch = 0; ch < ci; ++ch)
            for (int q = 0; q < P; ++q)
                HIPCHK(launch_pack_edge(dev_params + e->first_w + ((long long)32 * q * ci + ch) * 9, nullptr, ff + 288 * (ch * P + q), fb + 288 * (ch * P + q),
                                        nullptr, nullptr, s, 9 * ci));
        for (int o = 0; o < co; ++o)
            for (int q = 0; q < P; ++q)
                HIPCHK(launch_pack_edge(nullptr, dev_params + e->last_w + ((long long)o * nf + 32 * q) * 9, nullptr, nullptr, lf + 288 * (o * P + q),
                                        lb + 288 * (o * P + q), s));
    }
    for (auto& c : e->up) HIPCHK(launch_pack_shuffle_bias(dev_params + c.b_off, e->pk_sbias + c.sbias_off, e->planes, s));
    e->packed = true;
    return XSD_OK;
}

int xsd_forward(xsd_engine* e, const float* dev_x, float* dev_y, int B, int H, int W, int save_for_backward, void* stream)
{
    if (!e || !dev_x || !dev_y) return fail(XSD_ERR_ARG, "null argument");
    if (B < 1 || H < 1 || W < 1) return fail(XSD_ERR_ARG, "bad shape %dx%dx%d", B, H, W);
    if (!e->packed) return fail(XSD_ERR_STATE, "xsd_pack_weights must be called before xsd_forward");
    const int lo = e->cfg.kind == XSD_KIND_SR ? e->cfg.num_upsample : 0;
    if (e->generic) {
        const long long big = (long long)B * (H << lo) * (W << lo) * std::max(5 * e->cfg.num_filters, 4 * e->cfg.num_filters);
        if (big >= (1ll << 40)) return fail(XSD_ERR_ARG, "batch x image too large");
        hipError_t err = e->generic->forward(dev_x, dev_y, B, H, W, save_for_backward != 0, (hipStream_t)stream);
        if (err != hipSuccess) return fail(err == hipErrorOutOfMemory ? XSD_ERR_NOMEM : XSD_ERR_HIP, "generic-width forward: %s", hipGetErrorString(err));
        e->fwd_saved = save_for_backward != 0;
        return XSD_OK;
    }
    if ((long long)(H << lo) * (W << lo) * 32 >= (1ll << 31)) return fail(XSD_ERR_ARG, "image too large for 32-bit in-image offsets");
    // the split-mode kernels address a plane's batch slice with 32-bit BYTE offsets (buffer loads / stores): 128 B per pixel
    if (e->math >= 3 && (long long)(H << lo) * (W << lo) * 128 >= (1ll << 31))
        return fail(XSD_ERR_ARG, "image of %d x %d output pixels is too large for math modes bf16x6 / f16x3 (32-bit byte offsets: fewer than 2^24 pixels per image); use math mode fp32", H << lo, W << lo);
    if ((W << lo) > EDGE_MAX_W) return fail(XSD_ERR_ARG, "output rows wider than %d pixels are not supported", EDGE_MAX_W);
    int rc = ensure_plan(e, B, H, W, save_for_backward != 0);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    e->b_x = dev_x; e->b_y = dev_y;
    if (e->math == 4 && e->amax_used > 2) HIPCHK(hipMemsetAsync(e->amax + 2, 0, sizeof(float) * (e->amax_used - 2), s));   // every plane slot of the plan (forward and backward)
    for (auto& op : e->fwd_ops) HIPCHK(op(s));
    e->fwd_saved = save_for_backward != 0;
    return XSD_OK;
}

int xsd_backward_num_stages(const xsd_engine* e) { return e ? e->cfg.num_res_blocks + 2 : 0; }

int xsd_backward_stage(xsd_engine* e, int stage, const float* dev_dy, float* dev_dx_or_null, float* dev_grads, void* stream)
{
    if (!e || !dev_dy || !dev_grads) return fail(XSD_ERR_ARG, "null argument");
    if (!e->fwd_saved) return fail(XSD_ERR_STATE, "xsd_backward needs a preceding xsd_forward(save_for_backward=1)");
    if (e->generic) {
        if (stage < 0 || stage >= e->generic->num_stages()) return fail(XSD_ERR_ARG, "stage %d out of range", stage);
        hipError_t err = e->generic->backward_stage(stage, dev_dy, dev_dx_or_null, dev_grads, (hipStream_t)stream);
        if (err != hipSuccess) return fail(XSD_ERR_HIP, "generic-width backward stage %d: %s", stage, hipGetErrorString(err));
        return XSD_OK;
    }
    if (stage < 0 || stage >= (int)e->bwd_stages.size()) return fail(XSD_ERR_ARG, "stage %d out of range", stage);
    hipStream_t s = (hipStream_t)stream;
    e->b_dy = dev_dy; e->b_dx = dev_dx_or_null; e->b_grads = e->nf_pad ? e->grads_pad : dev_grads;
    // f16x3: the slots the backward launches report their planes' max |x| into (atomic max) start every backward at zero -- a
    // second backward after the same forward (another dy) must not inherit the first one's maxima (they would only over-
    // estimate, safe against fp16 overflow but costing operand bits)
    if (stage == 0 && e->math == 4 && e->amax_used > e->amax_bwd_first)
        HIPCHK(hipMemsetAsync(e->amax + e->amax_bwd_first, 0, sizeof(float) * (e->amax_used - e->amax_bwd_first), s));
    for (auto& op : e->bwd_stages[stage]) HIPCHK(op(s));
    if (e->nf_pad) {     // this stage's convs from the padded gradient into the caller's vector
        const int blocks = e->cfg.num_res_blocks;
        int d0, d1;
        if (stage == blocks + 1) { d0 = 0; d1 = 1; }                                   // conv_first
        else if (stage >= 1) { const int i = blocks - stage; d0 = 1 + 15 * i; d1 = d0 + 15; }   // dense blocks of rrdb.i
        else { d0 = 1 + 15 * blocks; d1 = e->npad; }                                  // trunk, conv_last, upsampling, HRconv
        HIPCHK(launch_pad_params(dev_grads, e->grads_pad, static_cast<const PadDesc*>(e->pad_descs) + d0, d1 - d0, 1, s));
    }
    return XSD_OK;
}

int xsd_backward(xsd_engine* e, const float* dev_dy, float* dev_dx_or_null, float* dev_grads, void* stream)
{
    const int n = xsd_backward_num_stages(e);
    for (int st = 0; st < n; ++st) {
        int rc = xsd_backward_stage(e, st, dev_dy, dev_dx_or_null, dev_grads, stream);
        if (rc) return rc;
    }
    return XSD_OK;
}

int xsd_grad_range(const xsd_engine* e, int stage, int range_idx, int64_t* offset, int64_t* count)
{
    if (!e) return 0;
    const int blocks = e->cfg.num_res_blocks;
    if (range_idx != 0 || stage < 0 || stage > blocks + 1) return 1;
    long long a, b;
    if (e->generic) {
        e->generic->grad_range(stage, &a, &b);
        if (offset) *offset = a;
        if (count) *count = b;
        return 1;
    }
    const std::vector<long long>& rb = e->nf_pad ? e->rrdb_begin_real : e->rrdb_begin;   // offsets in the caller's vector
    if (stage == 0) { a = rb[blocks]; b = e->nparams; }
    else if (stage <= blocks) { const int i = blocks - stage; a = rb[i]; b = rb[i + 1]; }
    else { a = 0; b = rb[0]; }
    if (offset) *offset = a;
    if (count) *count = b - a;
    return 1;
}

int xsd_l1_loss(xsd_engine* e, const float* dev_y, const float* dev_target, float* dev_dy_or_null, float* dev_loss, int64_t n, void* stream)
{
    if (!e || !dev_y || !dev_target || !dev_loss || n <= 0) return fail(XSD_ERR_ARG, "bad argument");
    HIPCHK(prof_launch(e, PK_LOSS, 0.0, (dev_dy_or_null ? 12.0 : 8.0) * n, (hipStream_t)stream, [&]() { return launch_l1_loss(dev_y, dev_target, dev_dy_or_null, e->loss_partial, 1024, dev_loss, n, (hipStream_t)stream); }));
    return XSD_OK;
}

struct xsd_loss_fn {
    LossWeights w;
    int channels = 1;        // images per sample (xsd_loss_set_channels)
    void* ws = nullptr;      // workspace, grown on demand
    size_t ws_bytes = 0;
};

int xsd_loss_create(const xsd_loss_config* cfg, xsd_loss_fn** out)
{
    if (!cfg || !out) return fail(XSD_ERR_ARG, "bad argument");
    LossWeights w;
    w.w[0] = cfg->w_l1; w.w[1] = cfg->w_poisson; w.w[2] = cfg->w_psnr; w.w[3] = cfg->w_ssim; w.w[4] = cfg->w_ms_ssim;
    w.correction = cfg->correction; w.sigma = cfg->sigma; w.k1 = cfg->k1; w.k2 = cfg->k2; w.kernel_size = cfg->kernel_size;
    bool any = false;
    for (int i = 0; i < 5; ++i) any = any || w.w[i] != 0.f;
    if (!any) return fail(XSD_ERR_ARG, "loss: no term has a non-zero weight");   // `assert metrics` (loss_functions.py:38)
    if ((w.w[3] != 0.f || w.w[4] != 0.f) && !(w.sigma > 0.f)) return fail(XSD_ERR_ARG, "loss: sigma must be > 0");
    xsd_loss_fn* f = new (std::nothrow) xsd_loss_fn();
    if (!f) return fail(XSD_ERR_NOMEM, "out of host memory");
    f->w = w;
    *out = f;
    return XSD_OK;
}

void xsd_loss_destroy(xsd_loss_fn* f)
{
    if (!f) return;
    xsd::dev_free(f->ws);
    delete f;
}

int xsd_loss_set_channels(xsd_loss_fn* f, int channels)
{
    if (!f || channels < 1 || channels > 1024) return fail(XSD_ERR_ARG, "xsd_loss_set_channels: channels must be 1..1024");
    f->channels = channels;
    return XSD_OK;
}

int xsd_loss_eval(xsd_loss_fn* f, const float* dev_y, const float* dev_target, float* dev_dy_or_null, float* dev_out8, int B, int H,
                  int W, void* stream)
{
    if (!f || !dev_y || !dev_target || !dev_out8) return fail(XSD_ERR_ARG, "bad argument");
    if (B < 1 || B % f->channels) return fail(XSD_ERR_ARG, "xsd_loss_eval: %d images are no whole number of %d-channel samples (xsd_loss_set_channels)", B, f->channels);
    const char* why = nullptr;
    if (loss_check(f->w, B, H, W, &why)) return fail(XSD_ERR_ARG, "%s", why);
    const size_t need = loss_workspace_bytes(B, H, W);
    if (need > f->ws_bytes) {
        HIPCHK(hipStreamSynchronize((hipStream_t)stream));
        if (f->ws) HIPCHK(xsd::dev_free(f->ws));
        f->ws = nullptr; f->ws_bytes = 0;
        if (xsd::dev_alloc(&f->ws, need) != hipSuccess) return fail(XSD_ERR_NOMEM, "loss workspace allocation failed");
        f->ws_bytes = need;
    }
    HIPCHK(launch_loss(f->w, dev_y, dev_target, dev_dy_or_null, dev_out8, B, f->channels, H, W, f->ws, (hipStream_t)stream));
    return XSD_OK;
}

int xsd_adam_step(xsd_engine* e, float* dev_params, const float* dev_grads, float* dev_m, float* dev_v, int64_t n, int step,
                  float lr, float beta1, float beta2, float eps, float grad_scale, void* stream)
{
    if (!dev_params || !dev_grads || !dev_m || !dev_v || n <= 0 || step < 1) return fail(XSD_ERR_ARG, "bad argument");
    auto go = [&]() { return launch_adam(dev_params, dev_grads, dev_m, dev_v, n, step, lr, beta1, beta2, eps, grad_scale, (hipStream_t)stream); };
    if (e) HIPCHK(prof_launch(e, PK_ADAM, 0.0, 28.0 * n, (hipStream_t)stream, go));      // reads p, g, m, v; writes p, m, v
    else HIPCHK(go());
    return XSD_OK;
}

int xsd_mask_pad_normalize(const void* dev_counts, int counts_is_int32, const uint8_t* dev_mask_or_null, float* dev_out, int B,
                           int Hin, int Win, int res, int do_normalize, float max_val, int stretch, void* stream)
{
    if (!dev_counts || !dev_out || B < 1 || Hin < 1 || Win < 1 || res < 1) return fail(XSD_ERR_ARG, "bad argument");
    if (stretch < 0 || stretch > 3) return fail(XSD_ERR_ARG, "stretch must be 0..3");
    if (do_normalize && !(max_val > 0.f)) return fail(XSD_ERR_ARG, "max_val must be > 0 on the fused path");
    MaskPadParams p; memset(&p, 0, sizeof(p));
    if (counts_is_int32) p.counts_i32 = (const int32_t*)dev_counts; else p.counts_f32 = (const float*)dev_counts;
    p.mask = dev_mask_or_null; p.out = dev_out; p.B = B; p.Hin = Hin; p.Win = Win; p.res = res;
    p.y_top = (int)std::floor((res - Hin) / 2.0); p.x_left = (int)std::floor((res - Win) / 2.0);
    p.do_norm = do_normalize; p.mode = stretch; p.max_val = max_val; p.upsample = 1;
    HIPCHK(launch_mask_pad_normalize(p, (hipStream_t)stream));
    return XSD_OK;
}

int xsd_compose_input(const void* dev_img, const void* dev_agn_or_null, const void* dev_bkg_or_null, int is_int32, int big_endian,
                      const uint8_t* dev_mask_or_null, float* dev_out, int B, int Hin, int Win, int upsample, int res,
                      int do_normalize, float max_val, int stretch, void* stream)
{
    if (!dev_img || !dev_out || B < 1 || Hin < 1 || Win < 1 || res < 1 || upsample < 1) return fail(XSD_ERR_ARG, "bad argument");
    if (stretch < 0 || stretch > 3) return fail(XSD_ERR_ARG, "stretch must be 0..3");
    if (do_normalize && !(max_val > 0.f)) return fail(XSD_ERR_ARG, "max_val must be > 0 on the fused path");
    MaskPadParams p; memset(&p, 0, sizeof(p));
    if (is_int32) p.counts_i32 = (const int32_t*)dev_img; else p.counts_f32 = (const float*)dev_img;
    p.extra1 = dev_agn_or_null; p.extra2 = dev_bkg_or_null; p.big_endian = big_endian; p.upsample = upsample;
    p.mask = dev_mask_or_null; p.out = dev_out; p.B = B; p.Hin = Hin; p.Win = Win; p.res = res;
    p.y_top = (int)std::floor((res - Hin * upsample) / 2.0); p.x_left = (int)std::floor((res - Win * upsample) / 2.0);
    p.do_norm = do_normalize; p.mode = stretch; p.max_val = max_val;
    HIPCHK(launch_mask_pad_normalize(p, (hipStream_t)stream));
    return XSD_OK;
}

int xsd_compose_batch(const void* dev_pool, int is_int32, int big_endian, int64_t slot_elems, int64_t n_slots,
                      const int32_t* img_idx, const int32_t* agn_idx_or_null, const int32_t* bkg_idx_or_null,
                      const uint8_t* dev_mask_or_null, float* dev_out, int B, int Hin, int Win, int upsample, int res,
                      int do_normalize, float max_val, int stretch, void* stream)
{
    if (!dev_pool || !img_idx || !dev_out || B < 1 || Hin < 1 || Win < 1 || res < 1 || upsample < 1 || n_slots < 1)
        return fail(XSD_ERR_ARG, "xsd_compose_batch: bad argument");
    if (slot_elems < (int64_t)Hin * Win) return fail(XSD_ERR_ARG, "xsd_compose_batch: slot of %lld words < Hin x Win = %d x %d", (long long)slot_elems, Hin, Win);
    if (stretch < 0 || stretch > 3) return fail(XSD_ERR_ARG, "stretch must be 0..3");
    if (do_normalize && !(max_val > 0.f)) return fail(XSD_ERR_ARG, "max_val must be > 0 on the fused path");
    // every index is checked here, before anything is launched: a bad one is an error that names the sample, never a device fault
    for (int b = 0; b < B; ++b) {
        if (img_idx[b] < 0 || img_idx[b] >= n_slots)
            return fail(XSD_ERR_ARG, "xsd_compose_batch: sample %d: img slot %d outside the pool's %lld slots", b, img_idx[b], (long long)n_slots);
        if (agn_idx_or_null && (agn_idx_or_null[b] < -1 || agn_idx_or_null[b] >= n_slots))
            return fail(XSD_ERR_ARG, "xsd_compose_batch: sample %d: agn slot %d outside the pool's %lld slots (-1 = absent)", b, agn_idx_or_null[b], (long long)n_slots);
        if (bkg_idx_or_null && (bkg_idx_or_null[b] < -1 || bkg_idx_or_null[b] >= n_slots))
            return fail(XSD_ERR_ARG, "xsd_compose_batch: sample %d: bkg slot %d outside the pool's %lld slots (-1 = absent)", b, bkg_idx_or_null[b], (long long)n_slots);
    }
    ComposeBatchParams p; memset(&p, 0, sizeof(p));
    p.pool = (const unsigned int*)dev_pool; p.mask = dev_mask_or_null; p.slot_elems = slot_elems;
    p.is_int32 = is_int32 != 0; p.big_endian = big_endian != 0;
    p.Hin = Hin; p.Win = Win; p.res = res; p.upsample = upsample;
    p.y_top = (int)std::floor((res - Hin * upsample) / 2.0); p.x_left = (int)std::floor((res - Win * upsample) / 2.0);
    p.do_norm = do_normalize; p.mode = stretch; p.max_val = max_val;
    for (int b0 = 0; b0 < B; b0 += COMPOSE_BATCH_CHUNK) {
        p.B = std::min(COMPOSE_BATCH_CHUNK, B - b0);
        p.out = dev_out + (int64_t)b0 * res * res;
        for (int b = 0; b < p.B; ++b) {
            p.img[b] = img_idx[b0 + b];
            p.agn[b] = agn_idx_or_null ? agn_idx_or_null[b0 + b] : -1;
            p.bkg[b] = bkg_idx_or_null ? bkg_idx_or_null[b0 + b] : -1;
        }
        HIPCHK(launch_compose_batch(p, (hipStream_t)stream));
    }
    return XSD_OK;
}

int xsd_normalize(const float* dev_in, float* dev_out, int64_t n, float max_val, int stretch, int inverse, void* stream)
{
    if (!dev_in || !dev_out || n <= 0 || !(max_val > 0.f) || stretch < 0 || stretch > 3) return fail(XSD_ERR_ARG, "bad argument");
    HIPCHK(launch_normalize(dev_in, dev_out, n, max_val, stretch, inverse, (hipStream_t)stream));
    return XSD_OK;
}

int xsd_image_upsample(const float* dev_in, float* dev_out, int N, int H, int W, int scale, void* stream)
{
    if (!dev_in || !dev_out || N < 1 || H < 1 || W < 1 || scale < 1) return fail(XSD_ERR_ARG, "bad argument");
    HIPCHK(launch_upsample_nearest(dev_in, dev_out, N, H, W, scale, (hipStream_t)stream));
    return XSD_OK;
}

int xsd_debug_persistent_grid(int ntiles, int ncu) { return (ntiles < 0 || ncu < 1) ? -1 : xsd::persistent_grid(ntiles, ncu); }
int xsd_debug_occupancy(int lds_bytes) { return xsd::debug_conv_occupancy(lds_bytes); }
float xsd_debug_residency_ms(int grid, int threads, int lds_bytes, int us) { return xsd::debug_residency_ms(grid, threads, lds_bytes, us); }

int xsd_probe_mfma_stream(int fmt, double seconds, double* mfma_tflops, double* sclk_ghz, void* stream)
{
    if ((fmt != 0 && fmt != 1) || !(seconds > 0.0) || seconds > 30.0 || !mfma_tflops)
        return fail(XSD_ERR_ARG, "xsd_probe_mfma_stream: fmt must be 0 (f16) or 1 (bf16), 0 < seconds <= 30, mfma_tflops non-NULL");
    HIPCHK(xsd::probe_mfma_stream(fmt, seconds, mfma_tflops, sclk_ghz, (hipStream_t)stream));
    return XSD_OK;
}

// diagnostic: accumulate shader-cycle stamps of the conv kernel's phases (enable != 0 allocates/zeroes; read copies out)
int xsd_debug_stamps(xsd_engine* e, int enable, unsigned long long* out16)
{
    if (!e) return fail(XSD_ERR_ARG, "null engine");
    HIPCHK(hipDeviceSynchronize());
    if (out16 && e->dbg) HIPCHK(hipMemcpy(out16, e->dbg, 32 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (enable) {
        if (!e->dbg && xsd::dev_alloc((void**)&e->dbg, 32 * sizeof(unsigned long long)) != hipSuccess)
            return fail(XSD_ERR_NOMEM, "xsd_debug_stamps: allocation of the stamp buffer failed");
        HIPCHK(hipMemset(e->dbg, 0, 32 * sizeof(unsigned long long)));
    } else if (e->dbg) { xsd::dev_free(e->dbg); e->dbg = nullptr; }
    return XSD_OK;
}

int xsd_profile_enable(xsd_engine* e, int enable)
{
    if (!e) return fail(XSD_ERR_ARG, "null engine");
    hipDeviceSynchronize();
    e->recs.clear(); e->ev_used = 0; e->prof = enable != 0;
    return XSD_OK;
}

int xsd_profile_read(xsd_engine* e, int klass, double* total_ms, int64_t* launches, double* total_flop, double* total_bytes)
{
    if (!e) return fail(XSD_ERR_ARG, "null engine");
    HIPCHK(hipDeviceSynchronize());
    double ms = 0, fl = 0, by = 0; int64_t n = 0;
    for (auto& r : e->recs) {
        if (r.klass != klass) continue;
        float t = 0.f;
        HIPCHK(hipEventElapsedTime(&t, r.a, r.b));
        ms += t; fl += r.flop; by += r.bytes; ++n;
    }
    if (total_ms) *total_ms = ms;
    if (launches) *launches = n;
    if (total_flop) *total_flop = fl;
    if (total_bytes) *total_bytes = by;
    return XSD_OK;
}

} // extern "C"
