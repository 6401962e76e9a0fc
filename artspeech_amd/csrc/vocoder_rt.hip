// Module-level C ABI of the HiFi-GAN generator (include/artspeech_hip.h, "The HiFi-GAN generator behind an opaque handle"): mel in,
// samples out, one call.  Like model.hip this file holds no kernels: it reads the checkpoint blob, lays the weights out (weight_norm
// fold, ConvTranspose1d -> 3-tap phase conv, per-row biases: checkpoint.h's host arithmetic; the fp32 conv_post row, the GEMM's weight
// images: uploads made here) and orders the launches of vocoder.hip / respair.hip / conv_gemm*.hip -- the sequence artspeech_amd/vocoder.py::Generator.forward_packed issues operator by
// operator, decision for decision.  ONE sequence (generator()), written against runtime.h's pass context like the acoustic model's,
// serves two passes: count (as_vocoder_workspace_bytes: the arena only adds up, nothing is launched) and run (kernels are enqueued;
// nothing is allocated, nothing synchronises once the geometry's tables exist) -- and two kinds of geometry: lengths the host knows
// (as_vocoder_forward: layouts cached in the plan) and lengths that exist on the device only (as_vocoder_forward_cap: capacity layouts
// whose tables lie in the workspace and are rewritten by every call's geometry launch).  as_vocoder_forward_windowed runs the capacity
// form round by round on windows of the mel (window.hip's gather in front, its stitch behind): the same sequence, a workspace sized by
// the window.
#include "common.h"
#include "conv_gemm.h"
#include "runtime.h"
#include "window_rule.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace asrt;

namespace {

constexpr float LRELU_SLOPE = 0.1f;     // Vocoder/vocoder.py:8
constexpr float POST_SLOPE = 0.01f;     // vocoder.py:111: F.leaky_relu's default
constexpr int ACT_LRELU = 2, ACT_TANH = 3;

struct ConvW : GemmW {                  // a conv weight prepared for as_conv_gemm_f32 / as_respair_f32, with its bias
    float* bias = nullptr;
};
struct Step {                           // one residual step of ResBlock1: conv1 (dilated), conv2
    ConvW c1, c2;
    int k = 0, dil = 1;
};

}  // namespace

struct as_vocoder {
    as_vocoder_cfg cfg;
    int device = 0, hop = 1;
    DevPool pool{(size_t)64 << 20};
    ConvW pre, post;                    // post.wh: only when the fp32 conv_post kernel does not apply
    float* post32 = nullptr;            // conv_post.weight[0] fp32 [C][k] (k = 3, 5, 7: as_conv_post_pcm_f32)
    int post_k = 0;
    std::vector<ConvW> ups;             // the phase convs [u Cout][Cin][3]; bias = the channel's, u times (one per row)
    std::vector<float*> ups_bias;       // the ConvTranspose1d's own bias [Cout] (as_interleave_phases_f32)
    std::vector<std::vector<Step>> rb;  // [stage * n_stacks + stack][step]
};

namespace {

using Raw = checkpoint::Map;

bool cfg_ok(const as_vocoder_cfg& c)
{
    if (c.num_mels <= 0 || c.upsample_initial_channel <= 0 || c.n_stages < 1 || c.n_stages > 8) return false;
    if (c.n_stacks != 3 || c.n_dilations < 1 || c.n_dilations > 4) return false;     // (the mean of THREE stacks: as_mean3_*_f32)
    if (c.upsample_initial_channel % (1 << c.n_stages)) return false;
    double hop = 1;
    for (int i = 0; i < c.n_stages; ++i) {
        const int u = c.upsample_rates[i];
        if (u < 2 || u > 4096 || c.upsample_kernel_sizes[i] != 2 * u) return false;
        hop *= u;
    }
    if (hop > (double)AS_META_MAX_W) return false;
    for (int j = 0; j < c.n_stacks; ++j) {
        const int k = c.resblock_kernel_sizes[j];
        if (k < 1 || !(k & 1) || k > AS_MAX_TAPS) return false;
        for (int n = 0; n < c.n_dilations; ++n)
            if (c.resblock_dilations[j][n] < 1 || c.resblock_dilations[j][n] > 4096) return false;
    }
    return true;
}

// every tensor the configuration names, with its shape (checkpoint.h) -- host work only: a bad checkpoint is refused before a device is
// touched
bool checkpoint_ok(const Raw& w, const as_vocoder_cfg& c)
{
    const checkpoint::GeneratorShape g = {c.num_mels, c.upsample_initial_channel, c.n_stages, c.n_stacks, c.n_dilations,
                                          c.upsample_kernel_sizes, c.resblock_kernel_sizes, AS_MAX_TAPS};
    std::string why;
    if (checkpoint::checkpoint_ok(w, g, &why)) return true;
    if (getenv("AS_DEBUG")) fprintf(stderr, "artspeech_hip: %s\n", why.c_str());
    return false;
}

float* upload(as_vocoder& v, const float* h, size_t n)
{
    float* d = static_cast<float*>(v.pool.alloc(n * sizeof(float)));
    if (!d || hipMemcpy(d, h, n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return d;
}

// w fp32 [Cout][Cin][T] -> the conv GEMM's weight image on the device (runtime.h: gemm_image), bias [n_bias] beside it
bool conv_w(as_vocoder& v, ConvW& g, const float* w, int Cout, int Cin, int T, const float* bias, size_t n_bias)
{
    if (gemm_image(v.pool, g, w, 1, Cout, Cin, T) != AS_OK) return false;
    g.bias = bias ? upload(v, bias, n_bias) : nullptr;
    return !bias || g.bias;
}
bool conv_w(as_vocoder& v, ConvW& g, const Raw& w, const std::string& name)
{
    const HostT &wt = w.at(name + ".weight"), &b = w.at(name + ".bias");
    return conv_w(v, g, wt.v.data(), wt.dim(0), wt.dim(1), wt.dim(2), b.v.data(), b.numel());
}

int vocoder_create(const void* blob_host, size_t blob_bytes, const as_vocoder_cfg* cfg, as_vocoder** out)
{
    Raw blob, w;
    if (!read_blob(blob_host, blob_bytes, &blob) || !fold(blob, &w)) return AS_EINVAL;
    blob.clear();
    if (!checkpoint_ok(w, *cfg)) return AS_EINVAL;
    struct Guard {                                                       // every error return below gives the device memory back
        std::unique_ptr<as_vocoder> v;
        ~Guard() { if (v) v->pool.release(); }
    } g;
    g.v.reset(new as_vocoder());
    as_vocoder& v = *g.v;
    v.cfg = *cfg;
    for (int i = 0; i < cfg->n_stages; ++i) v.hop *= cfg->upsample_rates[i];
    AS_CHECK(hipGetDevice(&v.device));
    bool ok = conv_w(v, v.pre, w, "conv_pre");
    const HostT &wp = w.at("conv_post.weight"), &bp = w.at("conv_post.bias");
    v.post_k = wp.dim(2);
    if (v.post_k == 3 || v.post_k == 5 || v.post_k == 7) {               // one output row: plain fp32 FMAs (vocoder.hip)
        v.post32 = upload(v, wp.v.data(), wp.numel());
        v.post.bias = upload(v, bp.v.data(), 1);
        ok = ok && v.post32 && v.post.bias;
    } else {
        ok = ok && conv_w(v, v.post, w, "conv_post");
    }
    v.ups.resize(cfg->n_stages);
    v.ups_bias.resize(cfg->n_stages);
    v.rb.resize((size_t)cfg->n_stages * cfg->n_stacks);
    for (int i = 0; ok && i < cfg->n_stages; ++i) {
        const std::string p = "ups." + std::to_string(i);
        const HostT &wt = w.at(p + ".weight"), &b = w.at(p + ".bias");
        const int u = cfg->upsample_rates[i], cin = wt.dim(0), cout = wt.dim(1);
        std::vector<float> wc((size_t)u * cout * cin * 3);
        const std::vector<float> rows = checkpoint::row_bias(b, u);
        ok = checkpoint::fold_upsample(wt.v.data(), cin, cout, u, wc.data());
        ok = ok && conv_w(v, v.ups[i], wc.data(), u * cout, cin, 3, rows.data(), rows.size());
        v.ups_bias[i] = upload(v, b.v.data(), b.numel());
        ok = ok && v.ups_bias[i];
        for (int j = 0; ok && j < cfg->n_stacks; ++j) {
            std::vector<Step>& blk = v.rb[(size_t)i * cfg->n_stacks + j];
            blk.resize(cfg->n_dilations);
            for (int n = 0; ok && n < cfg->n_dilations; ++n) {
                const std::string q = "resblocks." + std::to_string(i * cfg->n_stacks + j);
                blk[n].k = cfg->resblock_kernel_sizes[j];
                blk[n].dil = cfg->resblock_dilations[j][n];
                ok = conv_w(v, blk[n].c1, w, q + ".convs1." + std::to_string(n)) && conv_w(v, blk[n].c2, w, q + ".convs2." + std::to_string(n));
            }
        }
    }
    if (!ok) return (int)hipErrorOutOfMemory;
    AS_CHECK(hipDeviceSynchronize());
    *out = g.v.release();
    return AS_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// one pass over the launch sequence
// ------------------------------------------------------------------------------------------------------------------
// the shared pass context (runtime.h: arena, layout cache, device tables; Pass::Count and Pass::Run) plus the generator and the capacity
// form's workspace-resident layouts
struct Seq : PassCtx {
    const as_vocoder& v;
    Seq(const as_vocoder& v_, as_plan& p_, hipStream_t s_, void* ws, size_t ws_bytes, Pass pass_)
        : PassCtx(p_, s_, ws, ws_bytes, pass_, "vocoder_rt.hip"), v(v_) {}
    float* f32(int C, int N) { return PassCtx::f32((size_t)C * std::max(N, 1)); }

    // Capacity layouts (as_vocoder_forward_cap): rate i of {1, u0, u0 u1, ...} has cap * rate columns of ROOM; widths, offsets, column
    // descriptors and the valid count live in the WORKSPACE (AsVocGeo's two flat tables) and are written by the call's own geometry
    // launch -- nothing is cached, uploaded or allocated, so every call can be captured.  The Lay objects live as long as this pass.
    std::vector<std::unique_ptr<Lay>> caps;
    AsVocGeo geo;
    const Lay* cap_lays(int B, int cap, int max_len)
    {
        const as_vocoder_cfg& h = v.cfg;
        memset(&geo, 0, sizeof(geo));
        geo.B = B; geo.cap = cap; geo.max_len = max_len; geo.n_rates = h.n_stages + 1;
        long long rate = 1, cols = 0;
        for (int i = 0; i <= h.n_stages; ++i) {
            if (i) rate *= h.upsample_rates[i - 1];
            if ((double)rate * cap > 2147483647.0 || (double)rate * max_len > (double)AS_META_MAX_W) { fail(AS_EINVAL); return nullptr; }
            geo.rate[i] = (int32_t)rate;
            geo.meta_start[i] = cols;
            cols += rate * cap;
        }
        int32_t* tab = static_cast<int32_t*>(raw_alloc((size_t)geo.n_rates * (2 * B + 2) * sizeof(int32_t)));
        uint64_t* meta = static_cast<uint64_t*>(raw_alloc((size_t)cols * sizeof(uint64_t)));
        if (rc) return nullptr;
        geo.tab = tab;
        geo.meta = reinterpret_cast<unsigned long long*>(meta);
        for (int i = 0; i < geo.n_rates; ++i) {
            auto u = std::make_unique<Lay>();
            u->dyn = true; u->dyn_kind = i; u->dyn_B = B; u->cap1 = cap;
            u->B = B;
            u->N = geo.rate[i] * cap;
            u->max_w = geo.rate[i] * max_len;
            if (pass == Pass::Run) {
                u->d_w = tab + (size_t)i * (2 * B + 2);
                u->d_off = u->d_w + B;
                u->d_nvalid = u->d_w + 2 * B + 1;
                u->d_meta = meta + geo.meta_start[i];
            }
            caps.push_back(std::move(u));
        }
        return caps[0].get();
    }
    const Lay* scaled(const Lay* L, int k)
    {
        if (!L->dyn) return PassCtx::scaled(L, k);
        const size_t i = (size_t)L->dyn_kind + 1;
        if (i >= caps.size() || (long)caps[i]->N != (long)L->N * k) { fail(AS_EINVAL); return nullptr; }
        return caps[i].get();
    }
};

struct ConvOpt {
    const float* bias = nullptr;
    const float* res = nullptr;         // [M][N]
    int act = 0, in_act = 0;
    float in_slope = 0.2f;              // (what an unused slope is in the operator-level calls of vocoder.py: the GEMM ignores it)
    uint16_t* yh = nullptr;
    bool yh_lrelu = false;
    int ileave = 0, ldy = 0;            // ldy 0: lay->N
    int dil = 1;
};

// Y = epi(conv(W, X)): X fp32 [K][ldx] (the library splits it into the workspace) or the operand image xh; k taps with dilation o.dil
void conv(Seq& c, const ConvW& w, const float* X, int ldx, const uint16_t* xh, int K, const Lay* lay, float* Y, const ConvOpt& o)
{
    if (!lay || c.rc) return;
    if (K > w.Kp || K <= w.Kp - 16) { c.fail(AS_EINVAL); return; }
    ConvGemmArgs a;
    memset(&a, 0, sizeof(a));
    a.Wh = w.wh; a.X = X; a.Xh = xh; a.Y = Y; a.Yh = o.yh;
    a.bias = o.bias; a.res = o.res;
    a.M = w.M; a.N = lay->N; a.K = K; a.T = w.T; a.Kp = w.Kp;
    a.ldx = X ? ldx : lay->N; a.ldy = o.ldy ? o.ldy : lay->N; a.ldr = o.res ? lay->N : 0;
    a.act = o.act; a.in_act = o.in_act; a.yh_lrelu = o.yh_lrelu;
    a.acc_scale = 1.0f / w.scale;
    a.in_slope = o.in_slope; a.act_slope = 0.2f;
    a.n_prod = 3;
    a.n_groups = 1;
    a.ileave_u = o.ileave;
    for (int t = 0; t < w.T; ++t) { a.dh[t] = 0; a.dw[t] = o.dil * (t - w.T / 2); }
    if (lay->N == 0) return;
    // the workspace the library wants depends on WHICH operands are given, not on their addresses (null in the count pass)
    conv_gemm_rule::Shape sh = as_conv_gemm_shape(a);
    sh.x32 = !xh; sh.xh = xh != nullptr;
    const size_t wsb = as_conv_gemm_shape_workspace(sh, false);
    const size_t mark = c.off;
    a.ws = wsb ? c.raw_alloc(wsb) : nullptr;
    a.ws_bytes = wsb;
    c.off = mark;                                                       // (scratch of this launch only: the stream orders the next user behind it)
    if (!c.go()) return;
    a.meta = c.meta(lay);
    a.n_valid = lay->d_nvalid;                                          // (a capacity layout: the columns behind the utterances are filler)
    RUN(c, as_conv_gemm_f32(&a, c.s));
}

// Generator.forward (Vocoder/vocoder.py:101-113) on packed frames: the launch sequence of artspeech_amd/vocoder.py::forward_packed
// `lay`: the mel-rate layout -- Seq::lay (known lengths) or Seq::cap_lays (a capacity; lay->d_nvalid is then the device's valid count and
// every launch below is sized by the room, works on the valid columns and leaves the filler alone -- but for the last kernel, which
// writes the output's filler as 0)
void generator(Seq& c, const Lay* lay, const as_vocoder_io& io)
{
    const as_vocoder& v = c.v;
    const as_vocoder_cfg& h = v.cfg;
    const int nst = h.n_stages, nk = h.n_stacks, nd = h.n_dilations, c0 = h.upsample_initial_channel;
    if (!lay) return;
    if (c.pass == Pass::Run && io.ld_mel < lay->N) { c.fail(AS_EINVAL); return; }
    // what one stage hands to the next -- fp32 activations, or LeakyReLU of them as the next ConvTranspose1d's operand image -- lives in
    // one of two slots at the head of the arena (stage i reads slot i % 2 and writes the other); everything behind them is the stage's
    // own and is given back when the stage ends
    size_t slot_bytes = align256((size_t)c0 * std::max(lay->N, 1) * sizeof(float));
    {
        double n = lay->N;
        for (int i = 0; i < nst; ++i) {
            n *= h.upsample_rates[i];
            if (n > 2147483647.0) { c.fail(AS_EINVAL); return; }
            const int cout = c0 >> (i + 1), ni = std::max((int)n, 1);
            slot_bytes = std::max(slot_bytes, align256(std::max((size_t)cout * ni * sizeof(float), as_split_f16x2_bytes(cout, ni))));
        }
    }
    char* slot[2];
    for (int i = 0; i < 2; ++i) slot[i] = static_cast<char*>(c.raw_alloc(slot_bytes));
    if (c.rc) return;
    const size_t stage_base = c.off;

    float* x = reinterpret_cast<float*>(slot[0]);
    const uint16_t* xi = nullptr;       // LeakyReLU(x) as an operand image, when the producer of x wrote that instead of x
    {
        ConvOpt o;
        o.bias = v.pre.bias;
        conv(c, v.pre, io.mel, io.ld_mel, nullptr, h.num_mels, lay, x, o);
    }
    for (int i = 0; i < nst && !c.rc; ++i) {
        c.off = stage_base;
        const int u = h.upsample_rates[i], cin = c0 >> i, cout = c0 >> (i + 1);
        const Lay* lay_up = c.scaled(lay, u);
        if (!lay_up) return;
        const int N = lay_up->N;
        // ConvTranspose1d as one 3-tap conv with (phase, channel) rows: its epilogue stores the rows in time order when the channels are a
        // multiple of 32 (ConvGemmArgs.ileave_u); otherwise as_interleave_phases_f32 behind it
        const bool il = cout % 32 == 0;
        float* z = il ? c.f32(cout, N) : c.f32(u * cout, lay->N);
        ConvOpt o;
        if (il) { o.bias = v.ups[i].bias; o.ileave = u; o.ldy = N; }
        if (xi) {
            conv(c, v.ups[i], nullptr, 0, xi, cin, lay, z, o);
            xi = nullptr;
        } else {
            o.in_act = ACT_LRELU; o.in_slope = LRELU_SLOPE;
            conv(c, v.ups[i], x, lay->N, nullptr, cin, lay, z, o);
        }
        // 32 / 64 channels: the residual steps are fused launches; they address a tensor with 32-bit byte offsets
        const bool fused = (cout == 32 || cout == 64) && nk == 3 && 4.0 * u * cout * ((double)lay->N + 1.0) < 2147483648.0;
        if (il) {
            x = z;
        } else {
            x = c.f32(cout, N);
            RUN(c, as_interleave_phases_cap_f32(z, lay->N, v.ups_bias[i], cout, u, lay->N, lay->d_nvalid, x, N, c.s));
        }
        lay = lay_up;
        char* const out_slot = slot[(i + 1) & 1];
        const bool image_out = i + 1 < nst;                             // the stage's mean feeds only the next ConvTranspose1d
        float* outs[3] = {c.f32(cout, N), c.f32(cout, N), nullptr};
        if (fused) {
            // a residual step is ONE launch that keeps its column tile in LDS between the two convs; the stage's mean (and, between
            // stages, its LeakyReLU'd operand image) rides in the last step of the third stack
            float* tmp[2] = {c.f32(cout, N), c.f32(cout, N)};
            for (int j = 0; j < nk; ++j) {
                const float* y = x;
                const std::vector<Step>& blk = v.rb[(size_t)i * nk + j];
                for (int n = 0; n < nd; ++n) {
                    const bool end = n + 1 == nd, last = end && j + 1 == nk;
                    AsResPairArgs a;
                    memset(&a, 0, sizeof(a));
                    a.x = y; a.ldx = N;
                    if (last && image_out) { a.yh = reinterpret_cast<uint16_t*>(out_slot); a.yh_slope = LRELU_SLOPE; }
                    else { a.y = last ? reinterpret_cast<float*>(out_slot) : (end ? outs[j] : tmp[n & 1]); a.ldy = N; }
                    a.w1 = blk[n].c1.wh; a.w2 = blk[n].c2.wh; a.b1 = blk[n].c1.bias; a.b2 = blk[n].c2.bias;
                    a.scale1 = 1.0f / blk[n].c1.scale; a.scale2 = 1.0f / blk[n].c2.scale;
                    a.C = cout; a.N = N; a.k = blk[n].k; a.dil = blk[n].k > 1 ? blk[n].dil : 1; a.slope = LRELU_SLOPE;
                    a.col_off = lay->d_off; a.B = lay->B; a.max_w = lay->max_cols();
                    if (last) { a.add1 = outs[0]; a.add2 = outs[1]; a.ld_add = N; a.out_div = 3.0f; }
                    RUN(c, as_respair_f32(&a, c.s));
                    y = a.y;
                }
            }
            if (image_out) { x = nullptr; xi = reinterpret_cast<const uint16_t*>(out_slot); }
            else x = reinterpret_cast<float*>(out_slot);
            continue;
        }
        // LeakyReLU(x) as an operand image, once for the three stacks that start from x; inside a stack every conv hands its LeakyReLU'd
        // result to the next one as an image (ConvGemmArgs.Yh / yh_lrelu)
        outs[2] = c.f32(cout, N);
        uint16_t* xh = c.image(cout, N);
        RUN(c, as_split_f16x2_cap_f32(x, N, cout, N, lay->d_nvalid, ACT_LRELU, LRELU_SLOPE, xh, c.s));
        uint16_t* img[3] = {c.image(cout, N), c.image(cout, N), c.image(cout, N)};
        float* tmp[2] = {c.f32(cout, N), c.f32(cout, N)};
        for (int j = 0; j < nk; ++j) {
            const float* y = x;
            const uint16_t* yh = xh;
            const std::vector<Step>& blk = v.rb[(size_t)i * nk + j];
            for (int n = 0; n < nd; ++n) {
                const bool end = n + 1 == nd;
                uint16_t* xth = img[0];
                ConvOpt o1;
                o1.bias = blk[n].c1.bias; o1.yh = xth; o1.yh_lrelu = true; o1.in_slope = LRELU_SLOPE; o1.dil = blk[n].dil;
                conv(c, blk[n].c1, nullptr, 0, yh, cout, lay, nullptr, o1);
                uint16_t* next = end ? nullptr : img[1 + (n & 1)];
                float* yo = end ? outs[j] : tmp[n & 1];
                ConvOpt o2;
                o2.bias = blk[n].c2.bias; o2.res = y; o2.yh = next; o2.yh_lrelu = !end; o2.in_slope = LRELU_SLOPE;
                conv(c, blk[n].c2, nullptr, 0, xth, cout, lay, yo, o2);
                y = yo;
                yh = next;
            }
        }
        if (image_out) {
            RUN(c, as_mean3_image_cap_f32(outs[0], outs[1], outs[2], N, cout, N, lay->d_nvalid, LRELU_SLOPE, reinterpret_cast<uint16_t*>(out_slot), c.s));
            x = nullptr;
            xi = reinterpret_cast<const uint16_t*>(out_slot);
        } else {
            x = reinterpret_cast<float*>(out_slot);
            RUN(c, as_mean3_cap_f32(outs[0], outs[1], outs[2], N, cout, N, lay->d_nvalid, x, N, c.s));
        }
    }
    if (c.rc) return;
    // conv_post: LeakyReLU(0.01) -> one output row -> tanh, and the 16-bit samples in the same pass
    const int C = c0 >> nst, N = lay->N;
    if (v.post32) {
        const uint64_t* meta = c.meta(lay);
        RUN(c, as_conv_post_pcm_cap_f32(x, N, C, N, v.post32, v.post.bias, v.post_k, POST_SLOPE, 1, meta, lay->d_nvalid, io.wav, io.pcm, c.s));
    } else {
        float* wav = io.wav ? io.wav : c.f32(1, N);
        ConvOpt o;
        o.bias = v.post.bias; o.in_act = ACT_LRELU; o.in_slope = POST_SLOPE; o.act = ACT_TANH;
        conv(c, v.post, x, N, nullptr, C, lay, wav, o);
        // (under a capacity the GEMM stores nothing for the filler: this pass writes the zeros there, into wav too)
        if (io.pcm || lay->d_nvalid) RUN(c, as_pcm16_launch(wav, N, lay->d_nvalid, lay->d_nvalid && io.wav ? io.wav : nullptr, io.pcm, c.s));
    }
}

bool lens_ok(const as_vocoder* v, int B, const int32_t* lens, std::vector<int>* out)
{
    if (!v || B < 1 || !lens) return false;
    out->assign(lens, lens + B);
    for (int x : *out)
        if (x < 0 || (double)x * v->hop > (double)AS_META_MAX_W) return false;
    return true;
}

size_t count(const as_vocoder* v, as_plan* p, const std::vector<int>& lens, const as_vocoder_io& io, int* rc)
{
    Seq c(*v, *p, nullptr, nullptr, 0, Pass::Count);
    generator(c, c.lay(lens), io);
    *rc = c.rc;
    return c.rc ? 0 : c.peak + 256;
}

// the capacity form: the tables at the head of the arena, the geometry launch, then the same sequence
void generator_cap(Seq& c, int B, const as_vocoder_cap& g, const as_vocoder_io& io)
{
    const Lay* lay = c.cap_lays(B, g.cap, g.max_len > 0 ? g.max_len : g.cap);
    if (!lay) return;
    if (c.go()) {
        c.geo.off = g.off; c.geo.mult = g.mult; c.geo.sample_off = g.sample_off;
        c.geo.status = as_status_words_device();
        RUN(c, as_vocoder_cap_geometry_launch(c.geo, c.s));
    }
    generator(c, lay, io);
}

size_t count_cap(const as_vocoder* v, as_plan* p, int B, const as_vocoder_cap& g, const as_vocoder_io& io, int* rc)
{
    Seq c(*v, *p, nullptr, nullptr, 0, Pass::Count);
    generator_cap(c, B, g, io);
    *rc = c.rc;
    return c.rc ? 0 : c.peak + 256;
}

bool cap_ok(const as_vocoder* v, int B, int cap, int max_len)
{
    if (!v || B < 1 || B > 65535 || cap < 1 || max_len < 0 || max_len > cap) return false;
    return (double)v->hop * (max_len > 0 ? max_len : cap) <= (double)AS_META_MAX_W && (double)v->hop * cap <= 2147483647.0;
}

// ------------------------------------------------------------------------------------------------------------------
// windowed: rounds of gather -> generator_cap on the round's packed windows -> stitch (window_rule.h)
// ------------------------------------------------------------------------------------------------------------------
struct WinGeo {
    as_window_cfg w;            // halo resolved, hop the generator's
    int per, room;              // frames a window may have; frames of a round's buffers (B windows)
};

bool window_ok(const as_vocoder* v, int B, const as_window_cfg* w, WinGeo* out)
{
    if (!v || !w || B < 1 || B > 65535 || w->core < 1 || w->halo < -1) return false;
    const int halo = w->halo >= 0 ? w->halo : as_window_halo(&v->cfg);
    const double per = (double)w->core + 2.0 * halo;
    if (halo < 0 || per * v->hop > (double)AS_META_MAX_W || per * B * v->hop > 2147483647.0) return false;
    out->w = as_window_cfg{w->core, halo, v->hop};
    out->per = (int)per;
    out->room = (int)per * B;
    return cap_ok(v, B, out->room, out->per);
}

// The outer geometry of the windowed call: no utterance is ever laid out whole -- a round lays out core + 2 halo frames of it --, so the
// one-piece call's limit on an utterance's width (hop max_len <= AS_META_MAX_W) does not apply; sample positions stay 32-bit.
bool window_cap_ok(const as_vocoder* v, int B, int cap, int max_len)
{
    if (!v || B < 1 || B > 65535 || cap < 1 || max_len < 0 || max_len > cap) return false;
    return (double)v->hop * cap <= 2147483647.0;
}

// one round (the count pass: what any round needs).  The arena holds woff, the window mel and the window waveform in front of the
// capacity form's own tables and tensors: every round lays them out alike, and the stream orders a round behind the one before it.
void window_round(Seq& c, int B, const WinGeo& q, int round, const as_vocoder_cap* g, const as_vocoder_io* io)
{
    const as_vocoder& v = c.v;
    int32_t* woff = c.i32((size_t)B + 1);
    float* wmel = c.f32(v.cfg.num_mels, q.room);
    float* wwav = c.f32(1, (int)((long long)v.hop * q.room));
    if (c.rc) return;
    if (c.go())
        RUN(c, as_window_gather_launch(&q.w, round, io->mel, io->ld_mel, v.cfg.num_mels, g->off, B, g->mult, g->cap, g->max_len, wmel, q.room,
                                       woff, nullptr, false, c.s));
    const as_vocoder_cap inner = {woff, 1, q.room, q.per, nullptr};
    const as_vocoder_io wio = {wmel, q.room, wwav, nullptr};
    generator_cap(c, B, inner, wio);
    if (c.go())
        RUN(c, as_window_stitch_launch(&q.w, round, wwav, q.room, woff, g->off, B, g->mult, g->cap, g->max_len, io->wav, io->pcm,
                                       g->sample_off, false, c.s));
}

size_t count_windowed(const as_vocoder* v, as_plan* p, int B, const WinGeo& q, int* rc)
{
    Seq c(*v, *p, nullptr, nullptr, 0, Pass::Count);
    window_round(c, B, q, 0, nullptr, nullptr);
    *rc = c.rc;
    return c.rc ? 0 : c.peak + 256;
}

}  // namespace

extern "C" int as_vocoder_halo_cfg(const as_vocoder_cfg* cfg)
{
    if (!cfg || !cfg_ok(*cfg)) return AS_EINVAL;
    const int h = as_window_halo(cfg);
    return h < 0 ? AS_EINVAL : h;
}

extern "C" int as_vocoder_halo(const as_vocoder* v) { return v ? as_vocoder_halo_cfg(&v->cfg) : AS_EINVAL; }

extern "C" size_t as_vocoder_windowed_workspace_bytes(const as_vocoder* v, as_plan* p, int B, const as_window_cfg* w)
{
    WinGeo q;
    if (!p || !window_ok(v, B, w, &q)) return 0;
    size_t n = 0;
    (void)abi([&] { int rc; n = count_windowed(v, p, B, q, &rc); return rc; });
    return n;
}

extern "C" int as_vocoder_forward_windowed(const as_vocoder* v, as_plan* p, int B, const as_vocoder_cap* cap, const as_vocoder_io* io,
                                           const as_window_cfg* w, int round0, int n_rounds, void* ws, size_t ws_bytes, as_stream_t stream)
{
    if (!p || !cap || !io || !io->mel || (!io->wav && !io->pcm) || !cap->off || cap->mult < 1 || !window_cap_ok(v, B, cap->cap, cap->max_len))
        return AS_EINVAL;
    WinGeo q;
    if (!window_ok(v, B, w, &q) || round0 < 0 || n_rounds < 0 || io->ld_mel < cap->cap) return AS_EINVAL;
    if (!ws || misaligned(ws) || (io->pcm && (reinterpret_cast<uintptr_t>(io->pcm) & 1) != 0)) return AS_EINVAL;
    return abi([&] {
        hipStream_t s = static_cast<hipStream_t>(stream);
        int rc = enter(*p, s, ws, Pass::Run, false);                     // (no trim: the call touches no plan table)
        if (rc != AS_OK) return rc;
        // a workspace too small is refused before anything is launched
        const size_t need = count_windowed(v, p, B, q, &rc);
        if (rc != AS_OK) return rc;
        if (need > ws_bytes) return (int)AS_ENOSPC;
        const int all = window_rule::n_rounds(cap->max_len > 0 ? cap->max_len : cap->cap, q.w.core);
        const long long end = n_rounds > 0 ? std::min<long long>((long long)round0 + n_rounds, all) : all;
        for (long long r = round0; r < end; ++r) {
            p->next_event = 0;                                          // (rounds are ordered by the stream: each may use the plan's events again)
            Seq c(*v, *p, s, ws, ws_bytes, Pass::Run);
            window_round(c, B, q, (int)r, cap, io);
            if (c.rc) return c.rc;
        }
        return (int)AS_OK;
    });
}

extern "C" int as_vocoder_fold_upsample_host(const float* wt, int Cin, int Cout, int u, float* wc)
{
    if (!wt || !wc || Cin <= 0 || Cout <= 0 || u < 1) return AS_EINVAL;
    return checkpoint::fold_upsample(wt, Cin, Cout, u, wc) ? AS_OK : AS_EINVAL;
}

extern "C" int as_vocoder_create(const void* blob_host, size_t blob_bytes, const as_vocoder_cfg* cfg, as_vocoder** out)
{
    if (!blob_host || !cfg || !out || !cfg_ok(*cfg)) return AS_EINVAL;
    return abi([&] { return vocoder_create(blob_host, blob_bytes, cfg, out); });
}

extern "C" int as_vocoder_destroy(as_vocoder* v)
{
    if (!v) return AS_EINVAL;
    v->pool.release();
    delete v;
    return AS_OK;
}

extern "C" int as_vocoder_get_cfg(const as_vocoder* v, as_vocoder_cfg* out)
{
    if (!v || !out) return AS_EINVAL;
    *out = v->cfg;
    return AS_OK;
}

extern "C" int as_vocoder_hop(const as_vocoder* v) { return v ? v->hop : AS_EINVAL; }

extern "C" int as_vocoder_plan_create(const as_vocoder* v, as_plan** out)
{
    if (!v || !out) return AS_EINVAL;
    return abi([&] { *out = new as_plan(); return AS_OK; });
}

extern "C" size_t as_vocoder_workspace_bytes(const as_vocoder* v, as_plan* p, int B, const int32_t* lens_host)
{
    std::vector<int> lens;
    if (!p || !lens_ok(v, B, lens_host, &lens)) return 0;
    size_t n = 0;
    const as_vocoder_io io = {nullptr, 0, nullptr, nullptr};            // (no output given: the conv GEMM form of conv_post counts its fp32 row)
    (void)abi([&] { int rc; n = count(v, p, lens, io, &rc); return rc; });
    return n;
}

extern "C" int as_vocoder_forward(const as_vocoder* v, as_plan* p, int B, const int32_t* lens_host, const as_vocoder_io* io, void* ws,
                                  size_t ws_bytes, as_stream_t stream)
{
    std::vector<int> lens;
    if (!p || !io || !io->mel || (!io->wav && !io->pcm) || !lens_ok(v, B, lens_host, &lens)) return AS_EINVAL;
    if (!ws || misaligned(ws) || (io->pcm && (reinterpret_cast<uintptr_t>(io->pcm) & 1) != 0)) return AS_EINVAL;
    return abi([&] {
        hipStream_t s = static_cast<hipStream_t>(stream);
        int rc = enter(*p, s, ws, Pass::Run, true);
        if (rc != AS_OK) return rc;
        long total = 0;
        for (int x : lens) total += x;
        if (io->ld_mel < total) return (int)AS_EINVAL;
        if (total == 0) return (int)AS_OK;
        // a workspace too small is refused before anything is launched
        as_vocoder_io q = *io;
        q.wav = nullptr; q.pcm = nullptr;
        const size_t need = count(v, p, lens, q, &rc);
        if (rc != AS_OK) return rc;
        if (need > ws_bytes) return (int)AS_ENOSPC;
        Seq c(*v, *p, s, ws, ws_bytes, Pass::Run);
        generator(c, c.lay(lens), *io);
        return c.rc;
    });
}

extern "C" size_t as_vocoder_cap_workspace_bytes(const as_vocoder* v, as_plan* p, int B, int cap, int max_len)
{
    if (!p || !cap_ok(v, B, cap, max_len)) return 0;
    size_t n = 0;
    const as_vocoder_io io = {nullptr, 0, nullptr, nullptr};
    const as_vocoder_cap g = {nullptr, 1, cap, max_len, nullptr};
    (void)abi([&] { int rc; n = count_cap(v, p, B, g, io, &rc); return rc; });
    return n;
}

extern "C" int as_vocoder_forward_cap(const as_vocoder* v, as_plan* p, int B, const as_vocoder_cap* cap, const as_vocoder_io* io, void* ws,
                                      size_t ws_bytes, as_stream_t stream)
{
    if (!p || !cap || !io || !io->mel || (!io->wav && !io->pcm) || !cap->off || cap->mult < 1 || !cap_ok(v, B, cap->cap, cap->max_len))
        return AS_EINVAL;
    if (io->ld_mel < cap->cap) return AS_EINVAL;
    if (!ws || misaligned(ws) || (io->pcm && (reinterpret_cast<uintptr_t>(io->pcm) & 1) != 0)) return AS_EINVAL;
    return abi([&] {
        hipStream_t s = static_cast<hipStream_t>(stream);
        int rc = enter(*p, s, ws, Pass::Run, false);                     // (no trim: the call touches no plan table)
        if (rc != AS_OK) return rc;
        // a workspace too small is refused before anything is launched
        as_vocoder_io q = *io;
        q.wav = nullptr; q.pcm = nullptr;
        const size_t need = count_cap(v, p, B, *cap, q, &rc);
        if (rc != AS_OK) return rc;
        if (need > ws_bytes) return (int)AS_ENOSPC;
        Seq c(*v, *p, s, ws, ws_bytes, Pass::Run);
        generator_cap(c, B, *cap, *io);
        return c.rc;
    });
}
