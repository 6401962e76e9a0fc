// The checkpoint side of the module-level runtimes (model.hip: as_model_create; vocoder_rt.hip: as_vocoder_create) as host arithmetic
// alone: the "ASWBLOB1" reader, the weight_norm / spectral_norm fold, the twin-tower merge, and every assembly that turns folded
// tensors into the host arrays a weight image or an upload is made from (stacks, bias sums, a transpose, zero-padded columns, block
// diagonals, the ConvTranspose1d -> phase-conv rewrite).  Plain C++17 over standard headers: no HIP, no device, no cache -- the callers
// add the key, gemm_image / upload and the cache; tests/checkpoint_probe.cpp (compiled with g++, plain and under AddressSanitizer +
// UBSan) calls the same functions and tests/test_checkpoint_cpu.py holds every result to numpy, bit for bit.
//
// FAILURE.  Every function returns false when it cannot do its work.  One that looks tensors up takes `std::string* missing`: it
// receives the name of the FIRST tensor that was not found (find() keeps an earlier one) and stays empty when the failure is a shape.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

namespace checkpoint {

struct HostT {
    std::vector<int> dims;
    std::vector<float> v;
    size_t numel() const { return v.size(); }
    int dim(int i) const { return i < (int)dims.size() ? dims[i] : 1; }
};
using Map = std::unordered_map<std::string, HostT>;      // name -> tensor

// ------------------------------------------------------------------------------------------------------------------
// the blob, the folds, the twins
// ------------------------------------------------------------------------------------------------------------------
// the "ASWBLOB1" checkpoint format (include/artspeech_hip.h, as_model_create) -> name -> tensor; false: not a well-formed blob
inline bool read_blob(const void* blob, size_t bytes, Map* raw_out)
{
    // Every bound is checked in subtraction form against what is left (o <= bytes always holds): nothing here can wrap for any
    // header content, and nothing is allocated from a count the file merely claims.
    const unsigned char* b = static_cast<const unsigned char*>(blob);
    size_t o = 0;
    auto need = [&](size_t n) { return n <= bytes - o; };
    if (!need(12) || memcmp(b, "ASWBLOB1", 8) != 0) return false;
    o = 8;
    uint32_t n;
    memcpy(&n, b + o, 4);
    o += 4;
    if ((size_t)n > (bytes - o) / 11) return false;         // an entry is at least 2 + 0 + 1 + 0 + 8 bytes
    struct Ent { std::string name; std::vector<int> dims; uint64_t off; size_t numel; };
    std::vector<Ent> ents(n);
    for (uint32_t i = 0; i < n; ++i) {
        uint16_t nl;
        if (!need(2)) return false;
        memcpy(&nl, b + o, 2);
        o += 2;
        if (!need((size_t)nl + 1)) return false;
        ents[i].name.assign(reinterpret_cast<const char*>(b + o), nl);
        o += nl;
        const int nd = b[o++];
        if (nd > 8 || !need((size_t)nd * 4 + 8)) return false;
        size_t numel = 1;
        for (int d = 0; d < nd; ++d) {
            uint32_t v;
            memcpy(&v, b + o, 4);
            o += 4;
            if (v > (uint32_t)INT32_MAX) return false;
            if (v != 0 && numel > (SIZE_MAX / 4) / v) return false;   // numel * 4 must not wrap either
            numel *= v;
            ents[i].dims.push_back((int)v);
        }
        ents[i].numel = numel;
        memcpy(&ents[i].off, b + o, 8);
        o += 8;
    }
    uint64_t data_bytes;
    if (!need(8)) return false;
    memcpy(&data_bytes, b + o, 8);
    o += 8;
    if (data_bytes > bytes - o) return false;
    for (auto& e : ents) {
        if (e.off > data_bytes || e.numel * 4 > data_bytes - e.off) return false;
        HostT t;
        t.dims = e.dims;
        t.v.resize(e.numel);
        if (e.numel) memcpy(t.v.data(), b + o + e.off, e.numel * 4);
        (*raw_out)[e.name] = std::move(t);
    }
    return true;
}

inline bool ends_with(const std::string& s, const char* suf)
{
    const size_t n = strlen(suf);
    return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}

// weight_norm (torch old-style, dim 0): w = v * g / ||v|| over all dims but 0; spectral_norm in eval: w = W / (u . (W2d v))
// (artspeech_amd/weights.py is the Python statement of the same) -> plain "<prefix>.weight" tensors; plain
// tensors pass through; false: a part is missing
inline bool fold(const Map& in, Map* out)
{
    for (const auto& kv : in) {
        std::string k = kv.first;
        if (k.compare(0, 7, "module.") == 0) k = k.substr(7);
        if (k.compare(0, 30, "style_encoder.pitch_extractor.") == 0 || k.compare(0, 28, "style_encoder.ema_extractor.") == 0) continue;
        auto get = [&](const std::string& name) -> const HostT* {
            auto it = in.find(name);
            if (it == in.end()) it = in.find("module." + name);
            return it == in.end() ? nullptr : &it->second;
        };
        if (ends_with(k, ".weight_g")) {
            const std::string p = k.substr(0, k.size() - 9);
            const HostT* v = get(p + ".weight_v");
            if (!v || v->dims.empty() || kv.second.numel() != (size_t)v->dims[0]) return false;
            HostT w;
            w.dims = v->dims;
            w.v.resize(v->numel());
            const size_t rows = v->dims[0], per = v->numel() / rows;
            for (size_t r = 0; r < rows; ++r) {
                double s = 0;
                for (size_t i = 0; i < per; ++i) s += (double)v->v[r * per + i] * v->v[r * per + i];
                const float scale = kv.second.v[r] / (float)sqrt(s);
                for (size_t i = 0; i < per; ++i) w.v[r * per + i] = v->v[r * per + i] * scale;
            }
            (*out)[p + ".weight"] = std::move(w);
        } else if (ends_with(k, ".weight_orig")) {
            const std::string p = k.substr(0, k.size() - 12);
            const HostT *u = get(p + ".weight_u"), *vv = get(p + ".weight_v");
            const HostT& W = kv.second;
            if (!u || !vv || W.dims.empty() || u->numel() != (size_t)W.dims[0] || vv->numel() * W.dims[0] != W.numel()) return false;
            const size_t rows = W.dims[0], per = W.numel() / rows;
            double sigma = 0;
            for (size_t r = 0; r < rows; ++r) {
                double s = 0;
                for (size_t i = 0; i < per; ++i) s += (double)W.v[r * per + i] * vv->v[i];
                sigma += (double)u->v[r] * (double)(float)s;
            }
            HostT w;
            w.dims = W.dims;
            w.v.resize(W.numel());
            const float sg = (float)sigma;
            for (size_t i = 0; i < W.numel(); ++i) w.v[i] = W.v[i] / sg;
            (*out)[p + ".weight"] = std::move(w);
        } else if (ends_with(k, ".weight_v") || ends_with(k, ".weight_u")) {
            continue;
        } else {
            (*out)[k] = kv.second;
        }
    }
    return true;
}

// Two towers of the same architecture on different input channels (style_encoder.energy_block / F0_block + their Linear layers,
// models.py:402-411,414-415) as ONE tower of twice the width: every conv weight becomes block diagonal (the off-diagonal zeros multiply
// exactly to zero), depthwise weights and biases are concatenated.  Half the launches -- these 1-D towers are ~20 kernels of 8-10 us
// each, all at the fixed cost of a launch -- for twice the (negligible) flop.  Channel order: tower a first.
inline bool merge_twin_towers(Map* raw, const std::string& a, const std::string& b, const std::string& merged)
{
    std::vector<std::pair<std::string, HostT>> add;
    for (const auto& kv : *raw) {
        if (kv.first.compare(0, a.size() + 1, a + ".") != 0) continue;
        const std::string sfx = kv.first.substr(a.size());
        const auto itb = raw->find(b + sfx);
        if (itb == raw->end() || itb->second.dims != kv.second.dims) return false;
        const HostT &ta = kv.second, &tb = itb->second;
        HostT t;
        const bool is_w = sfx.size() >= 7 && sfx.compare(sfx.size() - 7, 7, ".weight") == 0;
        if (!is_w || sfx.find(".pool.") != std::string::npos) {           // bias / depthwise [C][1][k]: concatenate
            t.dims = ta.dims;
            t.dims[0] *= 2;
            t.v = ta.v;
            t.v.insert(t.v.end(), tb.v.begin(), tb.v.end());
        } else {                                                          // [Cout][Cin][k]: block diagonal
            const int co = ta.dim(0), ci = ta.dim(1), k = (int)(ta.numel() / ((size_t)co * ci));
            t.dims = ta.dims;
            t.dims[0] = 2 * co;
            t.dims[1] = 2 * ci;
            t.v.assign((size_t)4 * co * ci * k, 0.f);
            for (int m = 0; m < co; ++m)
                for (int c = 0; c < ci; ++c)
                    for (int j = 0; j < k; ++j) {
                        t.v[((size_t)m * 2 * ci + c) * k + j] = ta.v[((size_t)m * ci + c) * k + j];
                        t.v[((size_t)(co + m) * 2 * ci + ci + c) * k + j] = tb.v[((size_t)m * ci + c) * k + j];
                    }
        }
        add.emplace_back(merged + sfx, std::move(t));
    }
    if (add.empty()) return false;
    for (auto& kv : add) (*raw)[kv.first] = std::move(kv.second);
    return true;
}
// Linear layers of the twins -> one block Linear on [pooled a | pooled b] whose output rows are [rows of lb | rows of la] (the Style
// vector holds the F0 slice before the energy slice, models.py:423)
inline bool merge_twin_linears(Map* raw, const std::string& la, const std::string& lb, const std::string& merged)
{
    const auto wa = raw->find(la + ".weight"), wb = raw->find(lb + ".weight"), ba = raw->find(la + ".bias"), bb = raw->find(lb + ".bias");
    if (wa == raw->end() || wb == raw->end() || ba == raw->end() || bb == raw->end() || wa->second.dims != wb->second.dims) return false;
    const int o = wa->second.dim(0), i = wa->second.dim(1);
    HostT w, bias;
    w.dims = {2 * o, 2 * i};
    w.v.assign((size_t)4 * o * i, 0.f);
    for (int m = 0; m < o; ++m)
        for (int c = 0; c < i; ++c) {
            w.v[(size_t)m * 2 * i + i + c] = wb->second.v[(size_t)m * i + c];          // rows 0 .. o-1: lb on the second half of the input
            w.v[(size_t)(o + m) * 2 * i + c] = wa->second.v[(size_t)m * i + c];        // rows o .. : la on the first half
        }
    bias.dims = {2 * o};
    bias.v = bb->second.v;
    bias.v.insert(bias.v.end(), ba->second.v.begin(), ba->second.v.end());
    (*raw)[merged + ".weight"] = std::move(w);
    (*raw)[merged + ".bias"] = std::move(bias);
    return true;
}

// ------------------------------------------------------------------------------------------------------------------
// assemblies of the acoustic model: folded tensors in, host arrays out
// ------------------------------------------------------------------------------------------------------------------
// tensor `n`, or NULL with *missing = n unless an earlier lookup already failed
inline const HostT* find(const Map& m, const std::string& n, std::string* missing)
{
    const auto it = m.find(n);
    if (it != m.end()) return &it->second;
    if (missing->empty()) *missing = n;
    return nullptr;
}
inline void append(std::vector<float>* to, const HostT& t) { to->insert(to->end(), t.v.begin(), t.v.end()); }

// a weight [G][M][K][T] (+ [G][M][K2] behind the taps: a folded shortcut) with its bias [G][M], as gemm_image / upload take them
struct Mat {
    std::vector<float> w, w2, b;
    int G = 1, M = 0, K = 0, T = 1, K2 = 0;
};

// tensors `names` of one size one behind the other in `v`, `first` = the first of them; same_dims: of one shape too
inline bool concat(const Map& m, const std::vector<std::string>& names, bool same_dims, std::vector<float>* v, const HostT** first,
                   std::string* missing)
{
    *first = nullptr;
    for (const std::string& n : names) {
        const HostT* a = find(m, n, missing);
        if (!a) return false;
        if (!*first) *first = a;
        if (a->numel() != (*first)->numel() || (same_dims && a->dims != (*first)->dims)) return false;
        append(v, *a);
    }
    return *first != nullptr;
}
// conv weights `names`.weight ([Cout][Cin][k...] each, same shape) as the weight sets of one grouped launch
inline bool conv_stack(const Map& m, const std::vector<std::string>& names, Mat* o, std::string* missing)
{
    std::vector<std::string> w(names);
    for (std::string& n : w) n += ".weight";
    const HostT* a;
    if (!concat(m, w, true, &o->w, &a, missing)) return false;
    o->G = (int)names.size(); o->M = a->dim(0); o->K = a->dim(1); o->T = (int)(a->numel() / ((size_t)o->M * o->K));
    return true;
}
// the same with the shortcuts `sc_names`.weight ([Cout][Cin2][1]) behind the taps of every weight set
inline bool conv_fold(const Map& m, const std::vector<std::string>& names, const std::vector<std::string>& sc_names, Mat* o,
                      std::string* missing)
{
    const HostT *a = find(m, names[0] + ".weight", missing), *s0 = find(m, sc_names[0] + ".weight", missing);
    if (!a || !s0 || names.size() != sc_names.size()) return false;
    o->G = (int)names.size(); o->M = a->dim(0); o->K = a->dim(1); o->T = (int)(a->numel() / ((size_t)o->M * o->K)); o->K2 = s0->dim(1);
    for (size_t i = 0; i < names.size(); ++i) {
        const HostT *b = find(m, names[i] + ".weight", missing), *sc = find(m, sc_names[i] + ".weight", missing);
        if (!b || !sc || b->dims != a->dims || sc->dims != s0->dims || sc->dim(0) != o->M || sc->numel() != (size_t)o->M * o->K2) return false;
        append(&o->w, *b);
        append(&o->w2, *sc);
    }
    return true;
}
// q / k / v projections (`p`.conv_q|k|v, 1x1) of the attention layers `ps` as [G][3C][C] (RelTransformerEnc.py:128-133)
inline bool qkv(const Map& m, const std::vector<std::string>& ps, Mat* o, std::string* missing)
{
    for (const std::string& q : ps)
        for (const char* n : {"q", "k", "v"}) {
            const HostT* wt = find(m, q + ".conv_" + n + ".weight", missing);
            const HostT* bt = find(m, q + ".conv_" + n + ".bias", missing);
            if (!wt || !bt) return false;
            o->K = wt->dim(1);
            append(&o->w, *wt);
            append(&o->b, *bt);
        }
    o->G = (int)ps.size(); o->M = 3 * o->K;
    return true;
}
// nn.LSTM(bidirectional) `names` of one shape: the input projection of both directions as [G][8H][I], b_ih + b_hh per direction
inline bool lstm_wih(const Map& m, const std::vector<std::string>& names, Mat* o, std::string* missing)
{
    int H = 0;
    for (const auto& p : names) {
        const HostT *wi = find(m, p + ".weight_ih_l0", missing), *wir = find(m, p + ".weight_ih_l0_reverse", missing),
                    *bi = find(m, p + ".bias_ih_l0", missing), *bh = find(m, p + ".bias_hh_l0", missing),
                    *bir = find(m, p + ".bias_ih_l0_reverse", missing), *bhr = find(m, p + ".bias_hh_l0_reverse", missing);
        if (!wi || !wir || !bi || !bh || !bir || !bhr) return false;
        H = wi->dim(0) / 4;
        o->K = wi->dim(1);
        append(&o->w, *wi);
        append(&o->w, *wir);
        for (int i = 0; i < 4 * H; ++i) o->b.push_back(bi->v[i] + bh->v[i]);
        for (int i = 0; i < 4 * H; ++i) o->b.push_back(bir->v[i] + bhr->v[i]);
    }
    o->G = (int)names.size(); o->M = 8 * H;
    return true;
}
// W_hh of both directions transposed: [4H][H] each -> t [2][H][4H]
inline bool lstm_whh_t(const Map& m, const std::string& p, std::vector<float>* t, int* H_out, std::string* missing)
{
    const HostT *wh = find(m, p + ".weight_hh_l0", missing), *whr = find(m, p + ".weight_hh_l0_reverse", missing);
    if (!wh || !whr) return false;
    const int H = *H_out = wh->dim(1);
    t->resize((size_t)2 * H * 4 * H);
    for (int d = 0; d < 2; ++d) {
        const std::vector<float>& src = d ? whr->v : wh->v;
        for (int r = 0; r < 4 * H; ++r)
            for (int k = 0; k < H; ++k) (*t)[((size_t)d * H + k) * 4 * H + r] = src[(size_t)r * H + k];
    }
    return true;
}
// Every AdaIN fc layer fed by one style vector of K entries as ONE matrix [Mtot][K] (o->M = Mtot): `norms` = (layer name, first style
// entry it reads, entries it reads); a layer that reads a slice of the style (models.py:499,597-599) gets zero columns elsewhere.
// row0[name] = the layer's first output row.
struct NormSpec { std::string name; int off, S; };
inline bool fc_all(const Map& m, const std::vector<NormSpec>& norms, int K, Mat* o, std::unordered_map<std::string, int>* row0,
                   std::string* missing)
{
    o->K = K;
    for (const auto& n : norms) {
        const HostT *wt = find(m, n.name + ".fc.weight", missing), *bt = find(m, n.name + ".fc.bias", missing);
        if (!wt || !bt || wt->dim(1) != n.S || n.off + n.S > K) return false;
        const int M = wt->dim(0);
        (*row0)[n.name] = o->M;
        o->M += M;
        const size_t base = o->w.size();
        o->w.resize(base + (size_t)M * K, 0.f);
        for (int r = 0; r < M; ++r)
            for (int k = 0; k < n.S; ++k) o->w[base + (size_t)r * K + n.off + k] = wt->v[(size_t)r * n.S + k];
        append(&o->b, *bt);
    }
    return true;
}
// decoder.F0_conv (1 -> 32), N_conv (1 -> 32), EMA_conv (10 -> 64) (models.py:480-482, 1x1, weight-norm) as ONE block-diagonal
// 1x1 conv from the stacked [F0; N; EMA] rows (12) to the 128 channels the decoder concatenates (models.py:503-505)
inline bool fne(const Map& m, Mat* o, std::string* missing)
{
    const HostT *f = find(m, "decoder.F0_conv.weight", missing), *n = find(m, "decoder.N_conv.weight", missing),
                *e = find(m, "decoder.EMA_conv.weight", missing);
    const HostT *fb = find(m, "decoder.F0_conv.bias", missing), *nb = find(m, "decoder.N_conv.bias", missing),
                *eb = find(m, "decoder.EMA_conv.bias", missing);
    if (!f || !n || !e || !fb || !nb || !eb) return false;
    const int mf = f->dim(0), mn = n->dim(0), me = e->dim(0), ke = e->dim(1), K = o->K = 2 + ke;
    o->M = mf + mn + me;
    o->w.assign((size_t)o->M * K, 0.f);
    for (int r = 0; r < mf; ++r) o->w[(size_t)r * K + 0] = f->v[r];
    for (int r = 0; r < mn; ++r) o->w[(size_t)(mf + r) * K + 1] = n->v[r];
    for (int r = 0; r < me; ++r)
        for (int k = 0; k < ke; ++k) o->w[(size_t)(mf + mn + r) * K + 2 + k] = e->v[(size_t)r * ke + k];
    append(&o->b, *fb);
    append(&o->b, *nb);
    append(&o->b, *eb);
    return true;
}
// a Cin = 1 weight [Cout][1][T] as the direct kernel's fp32 image [T][Kp][Cout] (rows 1 .. Kp-1 of every tap: zero)
inline std::vector<float> direct_image(const float* w, int Cout, int T, int Kp)
{
    std::vector<float> w32((size_t)T * Kp * Cout, 0.f);
    for (int r = 0; r < Cout; ++r)
        for (int t = 0; t < T; ++t) w32[((size_t)t * Kp) * Cout + r] = w[(size_t)r * T + t];
    return w32;
}

// ------------------------------------------------------------------------------------------------------------------
// the HiFi-GAN generator's checkpoint
// ------------------------------------------------------------------------------------------------------------------
// the folded tensor `name` with exactly these dims, or NULL with *why = what is wrong with it
inline const HostT* tensor(const Map& w, const std::string& name, const std::vector<int>& dims, std::string* why)
{
    const auto it = w.find(name);
    if (it == w.end()) { *why = "vocoder checkpoint has no tensor '" + name + "'"; return nullptr; }
    if (it->second.dims != dims) { *why = "vocoder tensor '" + name + "' has another shape"; return nullptr; }
    return &it->second;
}
// what of as_vocoder_cfg names tensors (the arrays: n_stages and n_stacks entries); max_taps: the conv GEMM's AS_MAX_TAPS
struct GeneratorShape {
    int num_mels, c0, n_stages, n_stacks, n_dilations;
    const int32_t *upsample_kernel_sizes, *resblock_kernel_sizes;
    int max_taps;
};
// every tensor the configuration names, with its shape
inline bool checkpoint_ok(const Map& w, const GeneratorShape& c, std::string* why)
{
    const int c0 = c.c0;
    bool ok = tensor(w, "conv_pre.weight", {c0, c.num_mels, 7}, why) && tensor(w, "conv_pre.bias", {c0}, why);
    for (int i = 0; ok && i < c.n_stages; ++i) {
        const int cin = c0 >> i, cout = c0 >> (i + 1);
        const std::string p = "ups." + std::to_string(i);
        ok = tensor(w, p + ".weight", {cin, cout, c.upsample_kernel_sizes[i]}, why) && tensor(w, p + ".bias", {cout}, why);
        for (int j = 0; ok && j < c.n_stacks; ++j)
            for (int n = 0; ok && n < c.n_dilations; ++n)
                for (const char* cv : {".convs1.", ".convs2."}) {
                    const std::string q = "resblocks." + std::to_string(i * c.n_stacks + j) + cv + std::to_string(n);
                    ok = ok && tensor(w, q + ".weight", {cout, cout, c.resblock_kernel_sizes[j]}, why) && tensor(w, q + ".bias", {cout}, why);
                }
    }
    if (!ok) return false;
    const auto post = w.find("conv_post.weight");
    if (post == w.end()) { *why = "vocoder checkpoint has no tensor 'conv_post.weight'"; return false; }
    if (post->second.dims.size() != 3 || post->second.dim(0) != 1 || post->second.dim(1) != c0 >> c.n_stages || !(post->second.dim(2) & 1) ||
        post->second.dim(2) > c.max_taps) {
        *why = "vocoder tensor 'conv_post.weight' has another shape";
        return false;
    }
    return tensor(w, "conv_post.bias", {1}, why) != nullptr;
}
// ConvTranspose1d(k = 2u, stride u, padding u/2 + u%2) weight wt [Cin][Cout][2u] -> the 3-tap conv wc [u Cout][Cin][3] with (phase,
// channel) rows, taps x[q - 1], x[q], x[q + 1]; false: a phase needs a tap outside the three (no u >= 1 does)
inline bool fold_upsample(const float* wt, int Cin, int Cout, int u, float* wc)
{
    const int p = u / 2 + u % 2, k = 2 * u;
    memset(wc, 0, (size_t)u * Cout * Cin * 3 * sizeof(float));
    for (int r = 0; r < u; ++r) {
        const int rr = (r + p) % u, s = (r + p) / u;
        for (int j = 0; j < 2; ++j) {
            const int d = s - j + 1;                                    // taps x[q - 1], x[q], x[q + 1] = d 0, 1, 2
            if (d < 0 || d > 2) return false;
            for (int m = 0; m < Cout; ++m)
                for (int c = 0; c < Cin; ++c) wc[(((size_t)r * Cout + m) * Cin + c) * 3 + d] = wt[((size_t)c * Cout + m) * k + rr + u * j];
        }
    }
    return true;
}
// the phase conv's bias: the channel's, once per phase -- one entry per (phase, channel) row
inline std::vector<float> row_bias(const HostT& b, int u)
{
    std::vector<float> rows;
    for (int r = 0; r < u; ++r) append(&rows, b);
    return rows;
}

}  // namespace checkpoint
