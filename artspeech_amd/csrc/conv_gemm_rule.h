// What a conv GEMM call runs (conv_gemm.hip: conv_gemm) as a host-only rule: the direct Cin = 1 kernel or the tiled one, the tile, the K
// slices of each problem, the order of the problems inside a launch, whether the reduction of a K-sliced problem takes the AdaIN /
// LayerNorm behind it along, and how much workspace all that needs.  Plain C++17 over the C header's AS_MAX_MULTI: it sees a problem as a
// Shape -- dimensions, and booleans for which operands are given -- never a pointer into device memory, reads no environment (Force
// carries the four switches of tests and bench scripts) and calls neither HIP nor the library, so the count pass of a recorded plan, its
// run and a merged launch ask the same question and get the same answer -- tests/test_gemm_rule_cpu.py compiles it with g++ and holds
// it to the answers recorded in tests/golden/gemm_rule_parent.json.
//
// THE RULE.
//   Direct.  K = 1 from fp32 input with an fp32 weight, no second operand, residual, division, transposed or interleaved store or
//     weight groups, M <= 128, and an image out only with T <= 9: the direct kernel (one problem: any T; a set: every problem, T <= 9).
//   Tiles.  22 / 21 / 12 / 11 / 14 / 2 = 128x128, 128x64, 64x128, 64x64, 64x256, 32x128, four waves each.  The time of a launch is the
//     time of its busiest CU: a tile alone on a CU costs t1 (relative to 128x128: 128x64 / 64x128 0.78 -- they split K over wave pairs
//     and stage more per flop -- 64x64 0.59, 64x256 1.3), r > 1 rounds of 256 tiles cost 0.71 r t1 (two co-resident workgroups cover each
//     other's waits).  The cheapest tile wins; within 3 % the larger one does.  (Fitted to sweeps on MI355X, scripts/gemm_bench.py:
//     M512 N6400 K512 T3: 128x128 (200 tiles) 33.5 us, 128x64 (400) 37.1; M512 N3840 K512 T5: 44.8 (120 tiles) against 35.0 (240);
//     M512 N1280 K512 T3: 25.6 / 17.8 / 15.2 us for 40 / 80 / 160 tiles.  A 256x128 tile was measured and removed: DESIGN.md 3.1.)
//     M <= 32 everywhere: the 32-row tile (a 64-row tile would be half empty: HiFi-GAN's last stage, 32 channels, 1.9 M columns).
//     128-row tiles only for rows that fill them (fills_tall_tile).  Kp <= 32 never gets 64x64 but 64x128: an image of <= 32 channels
//     may come from the 32-row tile, which leaves the upper half of the image's 64-row block unwritten, and 64x64 is the one tile whose
//     waves read all four k-blocks of the block.
//     One problem and a set differ in three ways, kept as they were fitted (tile_one, tile_set):
//       64x256 -- one problem: M <= 64 and >= 240 tiles of N alone take it before any cost is compared (M64 N509440 K64 T9 167 -> 139 us,
//         N128000 41 -> 34, N63680 20.8 -> 19.7; below one round of the chip it loses: N6400 8.6 -> 10.8); a set: it competes in the table
//         at t1 = 1.3 once every problem has M <= 64 and the set >= 240 tiles;
//       weight groups -- count towards the tiles (groups x tiles of group_cols) only in a set;
//       tall -- one problem: its M fills the tall tile; a set: the problems whose M does carry >= 90 % of the set's work (a 64-channel
//         conv that rides along leaves the lower half of its few tiles empty, which costs less than a launch of its own).
//   K slices, one problem.  Only where even the smallest tiles leave most CUs idle: < 64 tiles: ceil(192 / tiles) slices, at most 16;
//     64 .. 128 tiles with >= 64 k-blocks of 16 (each workgroup alone on its CU, the k loop at the latency of its own staging): 512 / tiles.
//     A slice keeps >= 384 k (24 k-blocks over the waves_k waves that split K inside a workgroup).  An interleaved store is never sliced
//     (the slab reduction writes plain rows).  Slabs that do not fit the workspace: one slice.  fp32 input is split into an operand
//     image behind the slabs (256-byte aligned); no room for the image is an error.
//   K slices, a set.  A launch costs what its longest chain of k iterations on one CU costs.  With W = all problems' tiles x iterations
//     spread over the chip's 512 workgroup slots, a problem whose own chain is longer than 1.5 shares (the towers' closing 5 x 5 convs:
//     800 k-blocks on a dozen tiles, beside convs of 30 - 300) is cut into slices of about a share: at most 16, each >= 384 k, and no more
//     than its workspace holds slabs for.
//   Post slices.  A conv with an AdaIN / LayerNorm behind it that came out whole, reads an image, stores plain rows of <= 1 MB and has
//     >= 8 k-blocks is cut in TWO when the workspace holds two slabs and the reduction can write that normalisation (post_fits): the
//     reduction kernel then replaces the normalisation's launch.  Whatever the no_reduce switches say -- they change who normalises,
//     never the conv's own arithmetic.  (Two slices always have an iteration each: 8 k-blocks are >= 2 iterations of any tile.)
//   Fused.  The reduction of a K-sliced problem writes the normalisation's image itself (post_fused) when post_fits, the slabs stay
//     below 2^31 bytes x 16, the LayerNorm's parameters are aligned (the caller says) and no switch forbids it.
//   Order.  The problems of a set play longest slice (iterations / S) first; equal lengths keep the list's order.
//   Workspace.  workspace_one: the slabs plan_one wants with unlimited room, never less than the two slabs of a post slice, plus the
//     split image.  workspace_set: never less, and for an output of <= 4 MB read from an image up to 16 slabs, each slice >= 384 k.
#pragma once
#include "artspeech_hip.h"
#include "operand_image.h"
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace conv_gemm_rule {

constexpr int DIRECT_M = 128;                      // the direct kernel's weights in LDS
constexpr size_t POST_SLAB_MAX = (size_t)1 << 20;

// what the rule sees of one problem (of a normalised ConvGemmArgs: n_prod 1 / 3, n_groups >= 1)
struct Shape {
    int M = 0, N = 0, K = 0, Kp = 0, T = 0, K2 = 0, n_prod = 3, n_groups = 1, group_cols = 0, ileave_u = 0, act = 0;
    bool x32 = false, xh = false;                  // fp32 input given / operand image given
    bool y32 = false, yh = false;                  // fp32 output wanted / output image wanted
    bool w32 = false;                              // the fp32 Cin = 1 weight is there
    bool res = false, div_sqrt2 = false, transpose_out = false;
    bool has_ws = false;                           // a workspace is given, of ws_bytes
    size_t ws_bytes = 0;
};

// AS_GEMM_TILE, AS_GEMM_KSPLIT (> 0: that tile / that many slices wanted), AS_NO_REDUCE_ADAIN, AS_NO_REDUCE_LN
struct Force {
    int tile = 0, ksplit = 0;
    bool no_reduce_adain = false, no_reduce_ln = false;
};

// the normalisation that reads the conv's result
struct Post {
    enum Kind { None, Adain, Ln } kind = None;
    int max_w = 0;                                 // Adain: its widest utterance, columns
    bool ln_aligned = false;                       // Ln: gamma / beta / bias allow the reduction's 16-byte loads (the caller looks at the pointers)
};

struct Plan {
    bool ok = true;                                // false (the call is invalid): no room for the split image; a set the one launch cannot run
    bool direct = false;                           // the Cin = 1 kernel; nothing below is set
    int tile = 0;
    int S[AS_MAX_MULTI] = {}, order[AS_MAX_MULTI] = {};   // K slices of problem i; the k-th problem of the launch is order[k]
    bool fused[AS_MAX_MULTI] = {};                 // the reduction of problem i writes its Post
    size_t xh_off = 0;                             // one problem, fp32 input: its split image's offset in the workspace
};

inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }
inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }
constexpr int kbx(int K) { return operand_image::kbx(K); }             // the split image's k-blocks and size: operand_image.h
inline size_t split_f16x2_bytes(int K, int N) { return operand_image::bytes(K, N); }
inline size_t slab_bytes(const Shape& s) { return (size_t)s.M * s.N * sizeof(float); }
inline bool sized(const Shape& s) { return s.M > 0 && s.N > 0 && s.Kp > 0 && s.T > 0; }
// M output channels fill a 128-row tile well enough to use one (it is not half empty)
inline bool fills_tall_tile(int M) { return M > 64 && (M % 128 == 0 || M % 128 > 64 || M >= 512); }

inline void tile_dims(int tile, int* bm, int* bn)
{
    *bm = (tile == 22 || tile == 21) ? 128 : tile == 2 ? 32 : 64;
    *bn = tile == 14 ? 256 : (tile == 22 || tile == 12 || tile == 2) ? 128 : 64;
}
// waves that split K inside the workgroup
inline int waves_k(int tile)
{
    int bm, bn;
    tile_dims(tile, &bm, &bn);
    return tile == 2 ? 2 : bm * bn >= 4 * 64 * 64 ? 1 : 4 * 64 * 64 / (bm * bn);
}
// iterations of the k loop (a k-tile is 16 * wk); wk = 1: the k-blocks of 16
inline int k_iterations(const Shape& s, int wk) { return s.T * cdiv(s.Kp / 16, wk) + cdiv(cdiv(s.K2, 16), wk); }
inline int min_slice_iterations(int wk) { return std::max(1, 24 / wk); }     // a slice keeps >= 384 k
// tiles of one problem; grouped: every weight group has its own tiles over group_cols
inline double tiles_of(const Shape& s, int bm, int bn, bool grouped)
{
    return (double)cdiv(s.M, bm) * (grouped && s.n_groups > 1 ? s.n_groups * cdiv(s.group_cols, bn) : cdiv(s.N, bn));
}
inline double tile_cost(int tile, double tiles)
{
    const double t1 = tile == 22 ? 1.0 : tile == 14 ? 1.3 : tile == 11 ? 0.59 : 0.78;
    const double r = std::ceil(tiles / 256.0);
    return t1 * (r > 1.0 ? 0.71 * r : 1.0);
}
// the cheapest of the tiles offered, largest first: ties within 3 % go to the larger tile
struct Cheapest {
    int tile = 11;
    double cost = 1e30;
    void offer(int t, double tiles)
    {
        const double c = tile_cost(t, tiles);
        if (c < cost * 0.97) { cost = c; tile = t; }
    }
};

inline int tile_one(const Shape& s, const Force& f)
{
    if (f.tile > 0) return f.tile;
    if (s.M <= 32 && s.n_prod == 3) return 2;
    if (s.M <= 64 && s.n_prod == 3 && cdiv(s.N, 256) >= 240) return 14;          // (64x256: ahead of the table, by N alone)
    const bool tall = fills_tall_tile(s.M);                                      // (tall: this problem's rows)
    Cheapest best;
    for (int t : {22, 21, 12, 11}) {
        int bm, bn;
        tile_dims(t, &bm, &bn);
        if (bm >= 128 && !tall) continue;
        best.offer(t, tiles_of(s, bm, bn, false));                               // (weight groups do not count)
    }
    return s.Kp <= 32 && best.tile == 11 ? 12 : best.tile;
}

inline int tile_set(const Shape* s, int n, const Force& f)
{
    if (f.tile > 0) return f.tile;
    bool all_short = true, small_k = false, all_32 = true;
    double work = 0, tall_work = 0;
    for (int i = 0; i < n; ++i) {
        const double wi = (double)s[i].M * s[i].N * ((double)s[i].K * s[i].T + s[i].K2);
        work += wi;
        if (fills_tall_tile(s[i].M)) tall_work += wi;
        all_short = all_short && s[i].M <= 64;
        all_32 = all_32 && s[i].M <= 32;
        small_k = small_k || s[i].Kp <= 32;
    }
    const bool tall = tall_work >= 0.9 * work;                                   // (tall: by the share of the set's work)
    if (all_32 && s[0].n_prod == 3) return 2;
    Cheapest best;
    for (int t : {22, 21, 12, 11, 14}) {
        int bm, bn;
        tile_dims(t, &bm, &bn);
        if (bm >= 128 && !tall) continue;
        if (t == 14 && (!all_short || s[0].n_prod != 3)) continue;
        double tiles = 0;
        for (int i = 0; i < n; ++i) tiles += tiles_of(s[i], bm, bn, true);       // (weight groups count)
        if (t == 14 && tiles < 240) continue;                                    // (64x256: a row of the table)
        best.offer(t, tiles);
    }
    return small_k && best.tile == 11 ? 12 : best.tile;
}

inline bool direct_cin1(const Shape& s)
{
    return s.K == 1 && !s.K2 && s.w32 && s.x32 && (!s.yh || s.T <= 9) && !s.res && !s.div_sqrt2 && !s.transpose_out && s.ileave_u <= 1 &&
           s.M <= DIRECT_M && s.n_groups <= 1;
}

// can a reduction kernel write this normalisation?  (LayerNorm: a wave per column, a lane per 8 channels; AdaIN: a channel's whole time
// axis in <= 4 registers per lane)
inline bool post_fits(const Shape& s, const Post& p)
{
    if (s.act > 2) return false;
    if (p.kind == Post::Ln) return s.M % 8 == 0 && s.M <= 512 && !s.yh;
    return p.kind == Post::Adain && p.max_w > 0 && p.max_w <= 256;
}
inline bool post_fused(const Shape& s, const Post& p, const Force& f)
{
    return post_fits(s, p) && (double)s.M * s.N * 4.0 * 16.0 < 2147483648.0 &&
           (p.kind == Post::Ln ? p.ln_aligned && !f.no_reduce_ln : !f.no_reduce_adain);
}
inline bool post_slice_ok(const Shape& s)
{
    return s.xh && s.ileave_u <= 1 && !s.transpose_out && slab_bytes(s) <= POST_SLAB_MAX && k_iterations(s, 1) >= 8;
}
inline int post_slices(const Shape& s, int S, const Post& p)
{
    const bool two = S == 1 && post_slice_ok(s) && s.has_ws && s.ws_bytes >= 2 * slab_bytes(s) && post_fits(s, p);
    return two ? 2 : S;
}

inline int ksplit_one(const Shape& s, int tile, const Force& f)
{
    int bm, bn;
    tile_dims(tile, &bm, &bn);
    const long tiles = (long)cdiv(s.M, bm) * cdiv(s.N, bn);
    const int wk = waves_k(tile), nkt = k_iterations(s, wk);
    int S = 1;
    if (f.ksplit > 0) S = f.ksplit;
    else if (tiles < 64) S = std::min(cdiv(192, tiles), 16);
    else if (tiles <= 128 && nkt * wk >= 64) S = 512 / (int)tiles;
    return std::max(1, std::min(S, nkt / min_slice_iterations(wk)));
}

inline Plan plan_one(const Shape& s, const Post& post, const Force& f)
{
    Plan p;
    p.S[0] = 1;
    if (direct_cin1(s)) { p.direct = true; return p; }
    p.tile = tile_one(s, f);
    int S = s.ileave_u > 1 ? 1 : ksplit_one(s, p.tile, f);
    const size_t xh_bytes = s.xh ? 0 : split_f16x2_bytes(s.K, s.N), slabs = S > 1 ? S * slab_bytes(s) : 0;
    if (xh_bytes && (!s.has_ws || s.ws_bytes < xh_bytes)) { p.ok = false; return p; }
    const bool room = xh_bytes ? s.ws_bytes >= align256(slabs) + xh_bytes : s.has_ws && s.ws_bytes >= slabs;
    if (S > 1 && !room) S = 1;                                                   // no room for the slabs: no K slices
    p.xh_off = S > 1 ? align256(slabs) : 0;                                      // the split image goes behind the slabs
    p.S[0] = post_slices(s, S, post);
    p.fused[0] = p.S[0] > 1 && post_fused(s, post, f);
    return p;
}

inline Plan plan_set(const Shape* s, const Post* post, int n, const Force& f)
{
    Plan p;
    bool direct = true;
    for (int i = 0; i < n; ++i) direct = direct && direct_cin1(s[i]) && s[i].T <= 9;
    if (direct) { p.direct = true; return p; }
    // a set, in one launch: only what the tiled kernel runs from operand images with the same arithmetic
    for (int i = 0; i < n; ++i)
        if (direct_cin1(s[i]) || !s[i].xh || s[i].n_prod != s[0].n_prod || s[i].ileave_u > 1) { p.ok = false; return p; }
    p.tile = tile_set(s, n, f);
    int bm, bn;
    tile_dims(p.tile, &bm, &bn);
    const int wk = waves_k(p.tile);
    int nkt[AS_MAX_MULTI];
    double len[AS_MAX_MULTI], W = 0;
    for (int i = 0; i < n; ++i) {
        nkt[i] = k_iterations(s[i], wk);
        W += (double)nkt[i] * tiles_of(s[i], bm, bn, true);
    }
    const double share = std::max(W / 512.0, 1.0);
    for (int i = 0; i < n; ++i) {
        int S = nkt[i] > 1.5 * share ? (int)std::ceil(nkt[i] / share) : 1;
        S = std::min(std::min(S, 16), nkt[i] / min_slice_iterations(wk));
        if (S > 1) S = s[i].has_ws ? (int)std::min<size_t>(s[i].ws_bytes / slab_bytes(s[i]), (size_t)S) : 1;
        p.S[i] = post_slices(s[i], std::max(S, 1), post[i]);
        p.fused[i] = p.S[i] > 1 && post_fused(s[i], post[i], f);
        len[i] = (double)nkt[i] / p.S[i];
        p.order[i] = i;
    }
    std::stable_sort(p.order, p.order + n, [&](int x, int y) { return len[x] > len[y]; });
    return p;
}

// what one problem wants: its plan with room for everything and nothing behind it
inline Plan want_one(Shape s, const Force& f)
{
    s.has_ws = true;
    s.ws_bytes = SIZE_MAX / 2;
    return plan_one(s, Post(), f);
}

inline size_t workspace_one(const Shape& s, const Force& f)
{
    if (!sized(s)) return 0;
    const Plan p = want_one(s, f);
    if (p.direct) return 0;
    const size_t slabs = std::max(p.S[0] > 1 ? p.S[0] * slab_bytes(s) : 0, post_slice_ok(s) ? 2 * slab_bytes(s) : 0);
    const size_t xh_bytes = s.xh ? 0 : split_f16x2_bytes(s.K, s.N);
    return xh_bytes ? align256(slabs) + xh_bytes : slabs;
}

inline size_t workspace_set(const Shape& s, const Force& f)
{
    const size_t single = workspace_one(s, f);
    if (!sized(s) || !s.xh || slab_bytes(s) > ((size_t)4 << 20)) return single;   // (larger: tiles enough to never need slices)
    const int S = std::min(16, k_iterations(s, 1) / min_slice_iterations(1));
    return std::max(single, S > 1 ? S * slab_bytes(s) : 0);
}

}  // namespace conv_gemm_rule
