/*
 * libartspeech_hip.so -- C ABI of the MI355X-native ArtSpeech acoustic-model inference path.
 *
 * The reference (Zhongxu-Wang/ArtSpeech) is pure Python/PyTorch and has no FFI; its "operator API"
 * for this path is the Python call surface listed in SURVEY.md section 8(b).  Each entry point below
 * names the reference interface it replaces (file:line in the reference tree).  INTEGRATION.md
 * shows the ctypes binding a maintainer would add on the reference side.
 *
 * Conventions (all entry points)
 *   - extern "C", plain pointers and sizes; every pointer is a DEVICE pointer owned by the caller
 *     unless the parameter name ends in _host.
 *   - returns 0 on success, <0 for an invalid argument (AS_EINVAL = -1), >0 = a hipError_t.
 *   - never allocates, never synchronises, never throws: work is enqueued on `stream`
 *     (a hipStream_t passed as void*), scratch comes from a caller-provided workspace whose size
 *     the matching *_workspace_bytes() query returns.  Safe to capture in a hipGraph.
 *   - thread-safe for concurrent calls that use distinct streams and workspaces.
 */
#ifndef ARTSPEECH_HIP_H
#define ARTSPEECH_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void* as_stream_t; /* hipStream_t */

/* library/ABI version; bumped on any change of a signature or of a struct's layout (never held back for anything outside this header:
 * bench.py's source id of the kernel sources leaves version.hip out).  as_abi_version() returns the AS_ABI_VERSION the library was built
 * from: a caller compiled against another header must not go on (artspeech_amd/_lib.py refuses to). */
#define AS_ABI_VERSION 10
int as_abi_version(void);

/* Device-side status.  The reference's operators cannot return silently stale results: nn.Embedding raises on an id >= n_token
 * (RelTransformerEnc.py:11-16), cuDNN's LSTM (models.py:555-561) and the loops of S_monotonic_align.py:5-95 have no
 * cross-workgroup protocol that could time out.  Kernels of this library that can fail at run time raise a sticky bit instead of
 * carrying on unnoticed:
 *   bit AS_STATUS_LSTM_TIMEOUT  a member of a clustered H = 256 recurrence gave up waiting for its peers (as_bilstm_cluster_f32)
 *   bit AS_STATUS_MAS_TIMEOUT   a band of the alignment search gave up waiting for the band above it (as_mas_f32)
 *   bit AS_STATUS_BAD_TOKEN     a token id outside [0, n_token) reached the embedding (it was clamped)
 *   bit AS_STATUS_F16_RANGE     a conv GEMM produced a non-finite accumulator: an operand beyond fp16's range, |x| > 65504, or a
 *                               non-finite input (every launch under the debug probe as_set_range_probe; ALWAYS the last conv of
 *                               as_forward_test / as_decoder_forward, `to_out`: inf / NaN anywhere upstream reaches it -- every
 *                               ReLU of the library keeps a NaN, as torch.relu does -- so a non-finite mel is never handed back
 *                               silently)
 *   bit AS_STATUS_BAD_LAYOUT    an utterance wider than AS_META_MAX_W columns reached as_make_meta (its descriptors are void), an
 *                               utterance wider than the post_max_w its caller named -- or, with one utterance, another column range
 *                               than [0, N) -- reached as_conv_gemm_multi_post_f32's reduction, or (as_lanes_set_debug) the device
 *                               buffers of a submission changed while it was waiting for its group
 *   bit AS_STATUS_CAPACITY      the predicted durations of a batch (or of one submission of a merged call) add up to more frames than
 *                               the capacity its caller named (as_forward_io.frame_cap): what was computed was cut at the capacity --
 *                               nothing was written out of bounds, the mel is void; run it again with more room (the counterpart of
 *                               AS_ENOSPC where no host read-back tells the host in time)
 *   bit AS_STATUS_BAD_VOICE     a voice index outside [0, n_voices) reached a voice-mode forward (as_forward_io.voice_idx): that
 *                               utterance's Style and dur_style were set to zeros -- nothing was read out of bounds, its mel is void
 * as_device_status returns the bits raised on the current HIP device since the last clear (0 = healthy) without synchronising; it is
 * final for work whose stream has been synchronised.  The module-level entry points (as_*_forward, as_forward_test*) return
 * AS_EDEVICE while any bit is set: results computed since it was raised are invalid; clear it to go on. */
#define AS_EDEVICE (-3)
enum { AS_STATUS_LSTM_TIMEOUT = 0, AS_STATUS_MAS_TIMEOUT = 1, AS_STATUS_BAD_TOKEN = 2, AS_STATUS_F16_RANGE = 3, AS_STATUS_BAD_LAYOUT = 4,
       AS_STATUS_CAPACITY = 5, AS_STATUS_BAD_VOICE = 6, AS_STATUS_KINDS = 7 };
int as_device_status(int clear);
/* test hook: raise `kind` from a kernel on `stream`, exactly as a failing kernel would */
int as_device_status_raise_for_test(int kind, as_stream_t stream);
/* debug switch: activations are not range-scaled (only the weights are, as_prep_weight_f16x2_host), so a value beyond fp16's range
 * (|x| > 65504) enters its operand image as h = inf, l = -inf and turns every product it takes part in into NaN -- in the accumulators
 * of the conv GEMM that consumes the image.  on = 1 makes every as_conv_gemm_f32 launch test its accumulators and raise
 * AS_STATUS_F16_RANGE for a non-finite one (AS_DEBUG=1 in the environment also prints the launch's shape).  Off by default: the
 * test costs 16 compares per accumulator tile. */
int as_set_range_probe(int on);
#define AS_PROBE_THIS 2

/* Optional per-kernel-class timing with HIP events on the launch stream (bench.py's roofline leg; no
 * reference counterpart).  Classes: 0 conv-GEMM, 1 AdaIN, 2 LayerNorm, 3 attention, 4 LSTM, 5 MAS, 6 other.
 * as_prof_collect blocks until the recorded events have completed and returns, per class, the summed
 * kernel time (ms), algorithmic flop, algorithmic bytes and launch count since as_prof_enable(1). */
int as_prof_enable(int on);
int as_prof_collect(double* ms, double* flops, double* bytes, int32_t* launches, int n_classes);
/* algorithmic flop / bytes of the NEXT launch of this host thread, for entry points whose arguments do not determine them
 * (their geometry tables are device arrays); ignored while profiling is off */
int as_prof_hint(double flops, double bytes);
/* what one event bracket adds to the kernel inside it (ms): the command processor's work between the two markers, which a kernel
 * trace does not count.  Measured with brackets of 1, 2, 4, 8 empty kernels (the intercept); blocks. */
int as_prof_bracket_overhead(as_stream_t stream, double* overhead_ms);
/* what this device's matrix cores SUSTAIN on random fp16 operands (TFLOP/s of v_mfma_f32_32x32x16_f16): a bare loop of the conv GEMM's
 * own MFMA pattern with the operands in registers, and with them re-read from LDS at the GEMM's ratio (8 ds_read_b128 per 12 MFMAs).
 * The chip lowers its clock under matrix-core load on non-trivial data, so this -- not the data sheet's 2516.6 -- is what any kernel
 * can be compared with on this device.  Allocates and frees ~1.5 MB, blocks ~50 ms. */
int as_prof_mfma_sustained(as_stream_t stream, double* tflops_registers, double* tflops_lds_fed);

/* ---------------------------------------------------------------------------------------------
 * Monotonic alignment search (K1).
 * Replaces: maximum_path1  S_monotonic_align.py:5-47    (tie_mode = 1, "move")
 *           maximum_path2  S_monotonic_align.py:50-95   (tie_mode = 0, "stay")
 *           Triton maximum_path  S_monotonic_align_Triton.py:7-71 (tie_mode = 0)
 *           Cython wrapper  utils.py:11-24 (call surface; arithmetic source not in the tree)
 * value [B][Tx][Ty] fp32 (already masked or not: only the [t_x[b]) x [t_y[b]) corner is read; it is
 * never written).  t_x, t_y int32 [B] = valid text / mel lengths (what the reference recovers from
 * the mask at S_monotonic_align.py:15-16).
 * Outputs (each may be NULL): path fp32 [B][Tx][Ty] dense 0/1 (zero-filled here);
 * dur int32 [B][Tx] = path.sum(-1) (train_second.py:185); rows int32 [B][Ty] = text row of every mel
 * column, -1 past t_y[b].
 * ------------------------------------------------------------------------------------------- */
size_t as_mas_workspace_bytes(int B, int Tx, int Ty);
int as_mas_f32(const float* value, const int32_t* t_x, const int32_t* t_y, int B, int Tx, int Ty,
               int tie_mode, float* path, int32_t* dur, int32_t* rows,
               void* workspace, size_t workspace_bytes, as_stream_t stream);
/* The training scripts' producer of K1 in one call (train_second.py:181-184; train_first.py:171-177 without its masked_fill):
 * attn = softmax(feat, dim = softmax_dim) over the whole [Tx][Ty] slab (2 = the last axis, 1 = the Tx axis), then as_mas_f32 on
 * attn with the LENGTHS (what mask_from_lens + maximum_path do through a dense mask); dur = d_gt (train_second.py:185).
 * attn fp32 [B][Tx][Ty] is an output (s2s_attn is used downstream) and must not alias feat. */
int as_softmax_mas_f32(const float* feat, const int32_t* t_x, const int32_t* t_y, int B, int Tx, int Ty, int softmax_dim,
                       int tie_mode, float* attn, float* path, int32_t* dur, int32_t* rows, void* workspace,
                       size_t workspace_bytes, as_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Packed-frames layout (DESIGN.md "Data layout").  An activation is fp32 [C][N] (row stride ld >= N)
 * with every utterance of the batch concatenated along the contiguous column axis, no padding.
 * Column j carries a descriptor  h | H<<10 | w<<20 | W<<42  (AS_META_PACK: 10-bit rows, 22-bit columns): its (row, column)
 * inside its own utterance's H x W image (H = 1, w = frame index for 1-D sequences); H <= AS_META_MAX_H (mel bins),
 * W <= AS_META_MAX_W (the vocoder's last stage has 300 columns per mel frame: 174 s of audio per utterance).
 * as_make_meta builds the descriptors from per-utterance widths (int32 [B], device) for a common
 * height H; col_off int32 [B+1] are the utterances' first columns (exclusive prefix sums of H*W_b).  A width beyond
 * AS_META_MAX_W raises AS_STATUS_BAD_LAYOUT on the device (the widths are device data).
 * ------------------------------------------------------------------------------------------- */
#define AS_META_MAX_H 1023
#define AS_META_MAX_W 4194303
#define AS_META_PACK(h, w, H, W) \
    ((uint64_t)(h) | ((uint64_t)(H) << 10) | ((uint64_t)(w) << 20) | ((uint64_t)(W) << 42))
#define AS_META_h(md) ((int)((md) & 1023u))
#define AS_META_H(md) ((int)(((md) >> 10) & 1023u))
#define AS_META_w(md) ((int)(((md) >> 20) & 4194303u))
#define AS_META_W(md) ((int)((md) >> 42))
int as_make_meta(const int32_t* widths, const int32_t* col_off, int B, int H, int n_cols_max,
                 uint64_t* meta, as_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Dense convolution / linear layer as implicit GEMM on the matrix cores (K3, K4, K8, K10).
 *   Y[m][j] = epi( sum_t sum_k Wt[t][k][m] * X[k][j + dh[t]*W_j + dw[t]] ),   tap valid iff inside
 *   the column's own H x W image (zero padding otherwise).
 * Replaces nn.Conv1d (RelTransformerEnc.py:110-118,257-258,306-314; models.py:176-181,480-495,592-594),
 * nn.Conv2d 3x3/1x1 stride 1 (models.py:71-77,385-399,530-535) and nn.Linear over rows.
 * epi: *acc_scale, +bias[m], +res[m][j], /sqrt(2) (models.py:201, :100, :156), then act.
 *
 * Arithmetic ("f16x3"): every fp32 operand is split into two fp16 numbers, x = h + l (round-to-nearest-even twice: 22
 * significand bits), and a product is accumulated in fp32 from h*l + l*h + h*h on v_mfma_f32_32x32x16_f16 -- the dropped
 * l*l term is below 2^-22 |x w|.  Weights are scaled by a power of two before the split (as_prep_weight_f16x2 chooses it,
 * acc_scale undoes it) so that their l parts stay out of the fp16 subnormal range.  Operands must be finite and below
 * 65504 in magnitude.  n_prod = 1 keeps h*h only (plain fp16 operands: the "16-bit operand" mode of BASELINE.md C2).
 *
 * Operand images ("split images"), both staged global -> LDS by LDS-DMA in exactly this order:
 *   activations Xh [KBx][4][N+1][8] fp16: k-block kb = k/16, plane q = p*2 + kh holds part p (0 = h, 1 = l) of
 *       k = 16 kb + 8 kh + 0..7 for every column; column N is all zeros (where a tap outside the utterance reads);
 *       KBx = ceil(K/16) rounded up to a multiple of 4 (zero blocks).  4 bytes per element: the size of the fp32 tensor.
 *       Written by as_split_f16x2_f32, by the producers that feed only convolutions (as_adain_split_f32,
 *       as_channel_layernorm_split_f32, ...) or by the previous GEMM's epilogue (ConvGemmArgs.Yh).
 *   weights Wh [G][T][KBx][4][M][8] fp16 (as_prep_weight_f16x2), G = weight sets of a grouped launch.
 * ------------------------------------------------------------------------------------------- */
#define AS_MAX_TAPS 25
typedef struct ConvGemmArgs {
    const uint16_t* Wh;    /* split weights [G][T][KBx][4][M][8] fp16 */
    const float* W;        /* optional fp32 [T][Kp][M] image: only the Cin = 1 direct kernel reads it (K == 1 launches) */
    const float* X;        /* fp32 [K][ldx], or NULL when Xh is given */
    const uint16_t* Xh;    /* split activations [KBx][4][N+1][8] fp16 (in_act already applied by its writer), or NULL:
                              the library splits X into ws first (as_conv_gemm_workspace_bytes asks for the room) */
    float* Y;              /* fp32 [M][ldy] output, or NULL when only Yh is wanted */
    uint16_t* Yh;          /* optional: the output ALSO (or only) as the split image [KBy][4][N+1][8] of the convolution
                              that consumes it (KBy from M as KBx from K; rows >= M and column N zero) */
    const float* bias;     /* [G][M] or NULL */
    const float* res;      /* [M][ldr] or NULL (may alias Y) */
    const uint64_t* meta;  /* [N] column descriptors, or NULL = every tap valid */
    void* ws;              /* scratch: split-K partial slabs, then the split activations; NULL = neither */
    size_t ws_bytes;
    int32_t M, N, K, T;
    int32_t Kp;            /* K rounded up to a multiple of 16 (rows of zeros) */
    int32_t ldx, ldy, ldr;
    int32_t act;           /* epilogue activation: 0 none, 1 ReLU, 2 LeakyReLU(act_slope), 3 tanh, 4 |x| (Utils/JDC/model.py:137),
                              5 swish x*sigmoid(x) (Utils/EMA/conformer/conformer/activation.py:29) */
    int32_t div_sqrt2;     /* epilogue: divide by sqrt(2) after bias and residual (with act 0 - 2 only) */
    int32_t in_act;        /* 2 = LeakyReLU(in_slope) applied to X while it is split (models.py:89,142; Vocoder/vocoder.py:38,102);
                              ignored when Xh is given */
    int32_t transpose_out; /* 1 = write Y[j][m] (time-major, row stride ldy >= M); bias only: act 0, no div_sqrt2, res or Yh */
    int32_t yh_lrelu;      /* 1 = the image Yh holds LeakyReLU(in_slope)(y) (the consumer's in_act) while Y stays plain */
    int32_t n_prod;        /* 0 or 3 = f16x3 (fp32-accurate); 1 = h*h only */
    int32_t dh[AS_MAX_TAPS];   /* tap row offsets */
    int32_t dw[AS_MAX_TAPS];   /* tap column offsets */
    float in_slope, act_slope; /* LeakyReLU slopes of in_act / yh_lrelu and of act == 2, used exactly as given (the acoustic path's is
                                * AS_SLOPE_PATH = 0.2, models.py:163; nothing is substituted for 0: a slope of 0 IS ReLU); must be finite */
    float acc_scale;           /* multiplies the accumulator: 1 / (weight scale of as_prep_weight_f16x2); 0 = 1 */
    /* Grouped launch: G layers of the same shape side by side along the column axis (the text and articulatory encoders,
     * RelTransformerEnc.py; the F0 / energy / TV branches of ArtsPredictor, models.py:606-618): columns
     * [g * group_cols, (g+1) * group_cols) use weight set g.  n_groups <= 1: off. */
    int32_t n_groups, group_cols;
    int32_t range_probe;       /* AS_PROBE_THIS (2) from the caller: THIS launch tests its accumulators whatever as_set_range_probe says
                                * (as_forward_test's last conv: a non-finite mel always raises AS_STATUS_F16_RANGE); any other value is
                                * overwritten with as_set_range_probe's switch ... */
    uint32_t* status;          /* ... and the device's status words (as_device_status) */
    /* A 1x1 convolution of a SECOND operand summed into the same accumulators before the epilogue -- a residual block's learned
     * shortcut (models.py:79-84,185-186: conv1x1, no bias) evaluated by the launch of the block's last conv, as K2 more channels
     * of the reduction: Y = epi(sum_t W_t X(t) + W2 X2).  Xh2: split image [KBx2][4][N+1][8] of X2 (same N and column order as
     * Xh); its weights follow the T taps inside every weight set (as_prep_weight_f16x2_sc_host).  K2 = 0: none.  Needs Xh. */
    const uint16_t* Xh2;
    int32_t K2;
    /* Strided / valid convolutions (the 5x5 valid convs that close the 2-D towers, models.py:391,399,535): the OUTPUT columns are their
     * own layout (N of them) and output column j reads the input image at column src_col[j] + dh * W_in + dw, where meta[j] now
     * describes that INPUT position (h, w of tap (0, 0), H and W of the input image: taps outside it read zero) and Xh has N_in columns
     * (+ its zero column).  src_col NULL: off (the input is laid out like the output).  Needs Xh and meta; not with Xh2. */
    const int32_t* src_col;
    int32_t N_in;
    /* ileave_u >= 2: the M = ileave_u * C output rows are (phase r, channel m) -- row r C + m -- and Y is [C][ldy] with
     * Y[m][ileave_u * j + r] = result[r C + m][j]: a ConvTranspose1d(k = 2u, stride u) written as ONE 3-tap conv leaves in time order
     * (the interleave pass of as_interleave_phases_f32 folded into the store; the bias is given per ROW: the channel's, u times).
     * C a multiple of 32, ldy >= ileave_u * N; Y only (no Yh, res, transpose_out, weight groups); never K-sliced. */
    int32_t ileave_u;
    int32_t slab_tr;           /* library-owned (overwritten): the K slices' partial sums are stored time-major for a reduction that also
                                * computes the channel LayerNorm behind the conv (as_conv_gemm_multi_post_f32) */
    /* Capacity layouts (as_forward_io.frame_cap: the column count of a launch is a capacity, how many of the columns hold utterances is
     * known on the device only): *n_valid (a DEVICE int) = the leading columns that are valid -- of every weight group's column range when
     * the launch is grouped.  Columns behind them are filler: they read the zero column, nothing is stored for them, and a tile that lies
     * wholly in the filler ends at once, so a launch costs what its valid columns cost.  NULL: every column is valid. */
    const int32_t* n_valid;
} ConvGemmArgs;
#define AS_SLOPE_PATH 0.2f
int as_conv_gemm_f32(const ConvGemmArgs* args_host, as_stream_t stream);
/* Several INDEPENDENT convolutions (no problem reads what another writes) as ONE launch: the grid walks the tiles of all of them, longest
 * tiles first, so a problem that would own the chip alone at a fraction of its width -- the 40-tile convs of the duration predictor beside
 * the encoders' 240-tile ones, the small towers beside the mel tower: branches of ArtsSpeech.forward with no edge between them,
 * models.py:356-360, 417-424, 540-546 -- costs what it adds to the busiest CU, not a launch of its own.  Every problem as in
 * as_conv_gemm_f32 (own epilogue, groups, second operand, source positions), with these limits: operand images only (Xh given) and one
 * n_prod -- or a set made ONLY of Cin = 1 convs of <= 9 taps (the towers' stems: the direct kernel, one launch for the set); 1 <= n <=
 * AS_MAX_MULTI.  One tile shape serves the set (the cost model of the single launch on the
 * summed tile count: as_conv_gemm_multi_tile says which), so a problem's result can differ in the last bits from its single launch where
 * that one would have split K inside the workgroup -- same arithmetic, other order of the partial sums.  n == 1 is as_conv_gemm_f32. */
#define AS_MAX_MULTI 6
int as_conv_gemm_multi_f32(const ConvGemmArgs* list_host, int n, as_stream_t stream);
int as_conv_gemm_multi_tile(const ConvGemmArgs* list_host, int n);
/* workspace (ConvGemmArgs.ws) a problem wants when it may go into a multi-problem launch: a long reduction on a few tiles beside
 * shorter ones is cut into K slices there (as many as ws_bytes holds fp32 [M][N] slabs for) so that it does not outlast the launch;
 * >= as_conv_gemm_workspace_bytes */
size_t as_conv_gemm_multi_workspace_bytes(const ConvGemmArgs* args_host);
/* which kernel as_conv_gemm_f32 runs for these arguments (tests, tuning): *kind 0 = the direct Cin = 1 kernel, 1 = the tiled kernel
 * (*tile = 22 / 21 / 12 / 11 / 14 / 2: 128x128, 128x64, 64x128, 64x64, 64x256, 32x128); *slices = K slices */
int as_conv_gemm_plan(const ConvGemmArgs* args_host, int32_t* kind, int32_t* tile, int32_t* slices);
/* Bytes of workspace this shape wants (0 = none): split-K slabs for shapes whose tile grid cannot fill the 256 CUs (a second
 * kernel sums the slabs in a fixed order: deterministic), then the split image of X when Xh is NULL. */
size_t as_conv_gemm_workspace_bytes(const ConvGemmArgs* args_host);
/* X fp32 [K][ldx] (N columns) -> Xh (layout above).  in_act 2 applies LeakyReLU(in_slope) first (the slope as given).  One image can
 * feed every conv reading the same activations.  xh: 16-byte aligned, as_split_f16x2_bytes(K, N) bytes. */
size_t as_split_f16x2_bytes(int K, int N);
int as_split_f16x2_f32(const float* x, int ldx, int K, int N, int in_act, float in_slope, uint16_t* xh, as_stream_t stream);
/* The same under a capacity layout: *n_valid (a DEVICE int, NULL = N) leading columns are valid; columns [*n_valid, N) are filler that no
 * conv reads -- they are neither loaded nor converted (what xh holds there is left alone); the zero column N is written. */
int as_split_f16x2_cap_f32(const float* x, int ldx, int K, int N, const int32_t* n_valid, int in_act, float in_slope, uint16_t* xh,
                           as_stream_t stream);
/* Host-side weight preparation (no GPU work): w fp32 [G][Cout][Cin][T] (a folded nn.Conv / nn.Linear weight; T = product of
 * the kernel dims) -> wh [G][T][KBx][4][Cout][8] fp16 in HOST memory (as_prep_weight_f16x2_bytes(G, Cout, Cin, T) bytes),
 * scaled by *scale_out = the power of two that puts max |w| in [2^13, 2^14).  Pass ConvGemmArgs.acc_scale = 1 / *scale_out. */
size_t as_prep_weight_f16x2_bytes(int G, int Cout, int Cin, int T);
int as_prep_weight_f16x2_host(const float* w_host, int G, int Cout, int Cin, int T, uint16_t* wh_host, float* scale_out);
/* The same with the weights w2 fp32 [G][Cout][Cin2] of a 1x1 convolution on a second operand (ConvGemmArgs.Xh2 / K2) appended to every
 * weight set: wh [G][T * KBx + KBx2][4][Cout][8], one common scale.  Cin2 = 0 (w2 NULL): exactly the functions above. */
size_t as_prep_weight_f16x2_sc_bytes(int G, int Cout, int Cin, int T, int Cin2);
int as_prep_weight_f16x2_sc_host(const float* w_host, const float* w2_host, int G, int Cout, int Cin, int T, int Cin2, uint16_t* wh_host,
                                 float* scale_out);

/* ---------------------------------------------------------------------------------------------
 * Bandwidth-bound kernels on packed frames.  col_off int32 [B+1] = first column of each utterance.
 * ------------------------------------------------------------------------------------------- */
/* emb(x)*sqrt(C), transposed to [C][N]      RelTransformerEnc.py:373-374 */
int as_embed_f32(const int32_t* tokens, const float* emb, int C, int N, int V, float scale, float* y, int ldy,
                 as_stream_t stream);
/* the *_groups_* variants: column group g = column / n_split (utterance group g = utterance / b_split) takes parameter set
 * first + g * (second - first): two separately stored sets for two groups, or any number of equally spaced ones (a stack) -- encoders of the same
 * shape run as one double-width launch (ConvGemmArgs.n_groups is the GEMM's counterpart); NULL second set = the plain call */
/* as_embed_groups_f32: tokens holds n_tok ids.  n_tok == N: one id per column.  n_tok < N (the same tokens through every table):
 * column g * n_split + j reads tokens[j]; columns past n_tok inside a group are filler (id 0). */
int as_embed_groups_f32(const int32_t* tokens, int n_tok, const float* emb, const float* emb2, int n_split, int C, int N, int V,
                        float scale, float* y, int ldy, as_stream_t stream);
int as_channel_layernorm_groups_f32(const float* x, int ldx, int C, int N, const float* gamma, const float* beta, const float* gamma2,
                                    const float* beta2, int n_split, float eps, int relu, float* y, int ldy, as_stream_t stream);
/* Channel LayerNorm (+ReLU) written as the split operand image of the conv that follows (as_split_f16x2_f32's layout; pass it as
 * ConvGemmArgs.Xh): in the encoders a LayerNorm's output feeds nothing but that conv.  C <= 1024; second affine pair as above. */
int as_channel_layernorm_split_f32(const float* x, int ldx, int C, int N, const float* gamma, const float* beta, const float* gamma2,
                                   const float* beta2, int n_split, float eps, int relu, uint16_t* xs, as_stream_t stream);
int as_relpos_attention_groups_f32(const float* qkv, int ld, int C, int heads, int window, const float* emb_rel_k,
                                   const float* emb_rel_v, const float* emb_rel_k2, const float* emb_rel_v2, int b_split,
                                   const int32_t* col_off, int B, int max_len, float* out, int ldo, as_stream_t stream);
/* The same attention fed by the q/k/v projection's operand image (as_conv_gemm_f32 with Y and Yh: qkv fp32 [3C][ld] AND qkv_h, its image
 * over n_total columns): Q / K fragments come straight from the image, only V is read as fp32.  128-channel heads.  Writes out fp32
 * [C][ldo] and / or out_h, the operand image of the o-projection (n_total columns). */
int as_relpos_attention_image_f32(const float* qkv, int ld, const uint16_t* qkv_h, int n_total, int C, int heads, int window,
                                  const float* emb_rel_k, const float* emb_rel_v, const float* emb_rel_k2, const float* emb_rel_v2,
                                  int b_split, const int32_t* col_off, int B, int max_len, float* out, int ldo, uint16_t* out_h,
                                  as_stream_t stream);
/* no GPU work: the dynamic LDS bytes of a workgroup of the launch as_relpos_attention_image_f32 makes for this max_len (0 for
 * max_len <= 0).  max_len <= 64 takes the short-sequence form, of which three workgroups share a CU's 160 KB. */
int as_relpos_attention_image_lds_bytes(int max_len);
/* channel LayerNorm (eps 1e-4) (+ReLU)       RelTransformerEnc.py:272-290, :322-323 */
int as_channel_layernorm_f32(const float* x, int ldx, int C, int N, const float* gamma, const float* beta, float eps,
                             int relu, float* y, int ldy, as_stream_t stream);
/* AdaIN1d + LeakyReLU, per-utterance instance-norm statistics (biased var, eps 1e-5); gamma_beta [B][ldgb]
 * = fc(style) (gamma first).  With pool_w/pool_b [C][3]/[C] the depthwise ConvTranspose1d(k3,s2,p1,op1)
 * is fused: y gets 2x the frames (utterance b starts at 2*col_off[b]) and x_up (optional) the nearest-x2
 * copy of x.                                  models.py:189-197, 230-240, 172, 184, 261-270 */
int as_adain_f32(const float* x, int ldx, int C, const float* gamma_beta, int ldgb, const int32_t* col_off, int B,
                 float* y, int ldy, int lrelu, const float* pool_w, const float* pool_b, float* x_up, int ld_up,
                 as_stream_t stream);
/* The same AdaIN1d + LeakyReLU(0.2) written as the split operand image of the conv that follows (as_split_f16x2_f32's
 * layout, N = total columns; pass it as ConvGemmArgs.Xh): the fp32 activations are never stored. */
int as_adain_split_f32(const float* x, int ldx, int C, const float* gamma_beta, int ldgb, const int32_t* col_off, int B, int N,
                       int lrelu, uint16_t* xs, as_stream_t stream);
/* General form of the above (what the module-level entry points launch): per-utterance addressing of gamma / beta and of the
 * input columns, so that several layers of the same shape run as ONE launch on a grouped layout (the F0 / energy / TV branches of
 * ArtsPredictor, models.py:606-618) and read gamma / beta straight from a GEMM's [rows][utterances] output; optional fused
 * depthwise ConvTranspose1d x2 up-sampler (models.py:172,195) with the nearest-x2 copy of x as second output (models.py:184). */
typedef struct AsAdainArgs {
    const float* x;          /* [C][ldx] */
    int32_t ldx, C;
    const float* gb;         /* gamma(u, c) = gb[gb_off[u] + c * gb_sc], beta(u, c) = gb[gb_off[u] + (C + c) * gb_sc] */
    const int32_t* gb_off;   /* [U] float offsets; NULL = u * ldgb */
    int32_t ldgb, gb_sc;
    const int32_t* col_off;  /* [U + 1] OUTPUT columns of utterance u (times 2 with the up-sampler) */
    const int32_t* src_off;  /* [U] first INPUT column of utterance u; NULL = col_off[u] */
    int32_t U, N;            /* utterances; total output columns of the image (its zero column) */
    int32_t lrelu;
    uint16_t* yh;            /* the split image [KBx(C)][4][N+1][8] */
    const float* pool_w;     /* [C][3] depthwise ConvTranspose1d weights, or NULL = no up-sampling */
    const float* pool_b;     /* [C] */
    float* x_up;             /* optional [C][ld_up]: nearest x2 copy of x */
    int32_t ld_up;
    const int32_t* col_w;    /* optional [U]: utterance u has col_w[u] INPUT columns (times 2 out with the up-sampler) instead of col_off[u + 1] -
                              * col_off[u] -- layouts whose utterances do not lie back to back (capacity layouts: filler between groups) */
} AsAdainArgs;
int as_adain_image_f32(const AsAdainArgs* args_host, as_stream_t stream);
/* as_conv_gemm_multi_f32 for convolutions whose RESULT is (also) read through an AdaIN1d + LeakyReLU -- conv1 -> norm2 -> actv -> conv2
 * inside an AdainResBlk1d, conv2 -> the next block's norm1 (models.py:189-202) -- : problem i with post_host[i].yh != NULL also leaves
 * the operand image post[i].yh = split(LeakyReLU?(AdaIN(y_i))) over the utterances post[i].col_off [post[i].U + 1] of its N columns,
 * y_i = the conv's result after its own epilogue (post[i].x / ldx / C / N / src_off / pool_* are ignored: the input IS the conv's result,
 * list[i].Y must be given, C = M; gb / gb_off / ldgb / gb_sc / lrelu as in as_adain_image_f32).  What it buys: a launch that is cut into
 * K slices (few columns: batch 1, BASELINE config C2) ends in a reduction kernel that already holds a channel's whole time axis when no
 * utterance is wider than 256 columns (post_max_w[i] = the widest utterance of problem i), so that kernel computes the statistics and
 * writes the image itself -- conv -> reduce+AdaIN -> conv instead of conv -> reduce -> AdaIN -> conv, bit-identical to the separate
 * launches.  Everywhere else the call is exactly as_conv_gemm_multi_f32 followed by as_adain_image_f32 on list[i].Y.
 * post_host NULL: as_conv_gemm_multi_f32.  Not with transpose_out / ileave_u.  With ONE utterance (post[i].U == 1) the fused reduction
 * takes the utterance to be columns [0, N) without waiting for col_off; a col_off that says otherwise raises AS_STATUS_BAD_LAYOUT (the
 * two-launch form honours it: the two never differ silently).
 * The same for a conv whose result is read through a channel LayerNorm (+ ReLU) -- the encoders' conv -> residual add -> LayerNorm -> conv
 * (RelTransformerEnc.py:72-87, 318-325): problem i with post_ln_host[i].yh != NULL also leaves the operand image
 * yh = split(ReLU?(LayerNorm(y_i))) (as_channel_layernorm_split_f32's arithmetic and parameter addressing: column group g = column /
 * n_split takes gamma + g (gamma2 - gamma), NULL second set = one set).  K-sliced launches of <= 512 output channels (a multiple of 8)
 * store their partial sums time-major and the reduction kernel -- a wave per column -- writes the image itself; everywhere else the call
 * is the conv followed by as_channel_layernorm_split_f32 on list[i].Y.  post_ln_host NULL: none.  A problem has at most one of the two.
 * So that the fused form is the rule at batch 1, a conv with either normalisation behind it whose output is at most 1 MB is cut into two
 * K slices even where the slicing rules would leave it whole (as_conv_gemm_workspace_bytes / _multi_workspace_bytes leave room for the two
 * slabs of any such output): another order of two partial sums, the same arithmetic. */
typedef struct AsLnArgs {
    const float *gamma, *beta, *gamma2, *beta2;   /* [C] per set */
    int32_t n_split;
    float eps;
    int32_t relu;
    uint16_t* yh;                                  /* the split image [KBx(M)][4][N+1][8], or NULL: no LayerNorm behind this conv */
} AsLnArgs;
int as_conv_gemm_multi_post_f32(const ConvGemmArgs* list_host, const AsAdainArgs* post_host, const int32_t* post_max_w,
                                const AsLnArgs* post_ln_host, int n, as_stream_t stream);
/* x [B][ldx] (one K-vector per utterance) -> the split image of its transpose [K][B] (columns = utterances): the operand of
 * the GEMM that evaluates every AdaIN fc layer of the model at once (models.py:237). */
int as_rows_image_f32(const float* x, int ldx, int K, int B, uint16_t* xh, as_stream_t stream);
/* Y[m][j] = bias[m] + sum_k W[m][k] X[k][j] for a handful of output rows (M <= 16): the F0 / energy / TV projections behind the
 * BiLSTMs and duration_proj (models.py:565,619-621) -- bandwidth-bound, one column per thread. */
int as_project_cols_f32(const float* x, int ldx, int K, int N, const float* w, const float* bias, int M, float* y, int ldy,
                        as_stream_t stream);
/* Y[m][j] = bias[m] + sum_{k < K} W[m][k] X[k][j] for K <= 16 input channels (decoder.F0_conv / N_conv / EMA_conv as one block-diagonal
 * 12 -> 128 1x1 conv, models.py:480-482,503-505), written to up to two destinations, each as fp32 rows (y1 / y2, or NULL) and / or as the
 * rows of an operand image over N columns (yh1 / yh2: where the image's -- or a k-block-aligned part's -- first row group lives; rows
 * past M up to the image's 64-row block and the zero column N are written as zeros).  w fp32 [M][K]. */
int as_pointwise_small_f32(const float* x, int ldx, int K, int N, const float* w, const float* bias, int M, float* y1, int ld1,
                           uint16_t* yh1, float* y2, int ld2, uint16_t* yh2, as_stream_t stream);
/* y[b][m] = bias[m] + W[m][:] . x[b][:]       nn.Linear on per-utterance vectors (models.py:237,412-415,538) */
int as_linear_rows_f32(const float* x, int ldx, const float* w, const float* bias, int B, int M, int K, float* y,
                       int ldy, as_stream_t stream);
/* round-half-even + clamp(min=1) (or forced integer durations), per-utterance frame offsets [B+1] and the
 * frame -> token map; then the gather that replaces `T_en @ pred_aln_trg`.    models.py:361-368, :500 */
int as_durations_f32(const float* dur_f32, const int32_t* forced_dur, const int32_t* tok_off, int B, int32_t* dur_i32,
                     int32_t* frame_off, int32_t* tok_of_frame, int max_frames, as_stream_t stream);
int as_expand_f32(const float* x, int ldx, int C, const int32_t* tok_of_frame, int n_frames, int repeat, float* y,
                  int ldy, as_stream_t stream);
/* log_norm + stats.json normalisation; feat rows 0 = energy, 1 = f0, 2..11 = EMA.   models.py:431,447-449,655-660
 * stats24 = {energy_mean, energy_std, pitch_mean, pitch_std, EMA_mean[10], EMA_std[10]} */
int as_ref_features_f32(const float* mel, int ldm, int n_mels, const float* f0_raw, const float* ema_raw, int lde,
                        int N, const float* stats24, float* feat, int ldf, as_stream_t stream);
/* per-utterance column window copy (the T-1 crop, models.py:459-471) */
int as_crop_f32(const float* src, int lds, const int32_t* src_off, int start, float* dst, int ldd,
                const int32_t* dst_off, int B, int C, int max_len, as_stream_t stream);
/* H channel rows -> per-utterance H x W images packed [1][sum H*W_b] (img_off = the image layout's column offsets):
 * dst[img_off[b] + h*W_b + i] = src[h][src_off[b] + start + i]       the 2-D towers' inputs, models.py:419-421 */
int as_rows_to_images_f32(const float* src, int lds, const int32_t* src_off, int start, int H, float* dst,
                          const int32_t* img_off, int B, int max_w, as_stream_t stream);
/* style-tower helpers: LearnedDownSample / ResBlk1d.pool (models.py:27-31,116), DownSample (+ residual merge,
 * models.py:43-57,99-100,127-130), im2col for the valid KxK convs (models.py:391,399,535), LeakyReLU+avg-pool */
int as_dwconv_down_f32(const float* x, int ldx, const int32_t* in_off, const int32_t* in_w, int Hin, float* y, int ldy,
                       const int32_t* out_off, const int32_t* out_w, int Hout, const float* w, const float* bias,
                       int kh, int B, int C, int max_out, int lrelu, as_stream_t stream);
/* JDCNet's BatchNorm2d (eval: y = x*scale[c] + shift[c]) -> LeakyReLU(slope) -> MaxPool2d over the mel axis by k, floor
 * mode (Utils/JDC/model.py:29-34,166-170).  Images are [H rows = mel bins][W = frames of the utterance]; tok_off int32
 * [B+1] = first frame of each utterance in a 1-D layout, image b starts at column H*tok_off[b].  Output: images of
 * Hout = H / k rows (to_channels = 0), or the 1-D layout with C*Hout rows, row c*Hout + h (to_channels = 1: the
 * permute(0,2,1,3).view(.., 512) of model.py:126). */
int as_bn_lrelu_maxpool_rows_f32(const float* x, int ldx, const int32_t* tok_off, int B, int C, int H, int k, const float* scale,
                                 const float* shift, float slope, float* y, int ldy, int to_channels, int total_frames,
                                 as_stream_t stream);
int as_avgpool_down_f32(const float* x, int ldx, const int32_t* in_off, const int32_t* in_w, int Hin, float* y, int ldy,
                        const int32_t* out_off, const int32_t* out_w, int Hout, int pool_h, const float* res, int ldr,
                        int B, int C, int max_out, as_stream_t stream);
int as_im2col_valid_f32(const float* x, int ldx, const int32_t* in_off, const int32_t* in_w, int Hin, float* col,
                        int ldc, const int32_t* out_off, const int32_t* out_w, int Hout, int K, int stride, int lrelu,
                        int B, int C, int max_out, as_stream_t stream);
/* The producers above writing the split operand image of the conv that consumes them instead of (or, avgpool: beside) the fp32
 * tensor: yh [KBx(C)][4][n_out + 1][8] over the n_out packed output columns (as_split_f16x2_f32's layout).  yh_lrelu: the image
 * holds LeakyReLU(0.2)(y) -- the consumer's input activation (models.py:89,142) -- while y (optional) stays plain. */
int as_dwconv_down_image_f32(const float* x, int ldx, const int32_t* in_off, const int32_t* in_w, int Hin, const int32_t* out_off,
                             const int32_t* out_w, int Hout, const float* w, const float* bias, int kh, int B, int C, int max_out,
                             int lrelu, uint16_t* yh, int n_out, as_stream_t stream);
int as_avgpool_down_image_f32(const float* x, int ldx, const int32_t* in_off, const int32_t* in_w, int Hin, float* y, int ldy,
                              const int32_t* out_off, const int32_t* out_w, int Hout, int pool_h, const float* res, int ldr, int B,
                              int C, int max_out, uint16_t* yh, int n_out, int yh_lrelu, as_stream_t stream);
/* avgpool_down(stem(x)) for a tower's Cin = 1 stem conv (models.py:385,393 followed by the first block's shortcut, :79-84), from the
 * ONE-channel input x [sum H*W_b]: w = the stem's fp32 weight image [T][Kp][C] (row k = 0; T = 3 kh taps in taps_2d(3, 3) / taps_1d(3)
 * order), bias [C] or NULL, zero padding; (pool_h x 2) average with the last column replicated for odd widths; result as the operand
 * image yh over the n_out pooled columns.  The stem's own fp32 output is then never needed. */
int as_stem_pool_image_f32(const float* x, const int32_t* in_off, const int32_t* in_w, int Hin, const int32_t* out_off,
                           const int32_t* out_w, int Hout, int pool_h, const float* w, int Kp, const float* bias, int kh, int B, int C,
                           int max_out, uint16_t* yh, int n_out, as_stream_t stream);
/* One launch for up to AS_MAX_MULTI of the down-sampling steps above (independent problems: the style towers and dur_block march through
 * their ResBlks in step, models.py:385-411,530-535).  kind 0 = as_dwconv_down[_image]_f32 (w [C][kh*3], bias [C], lrelu = LeakyReLU on the
 * result), 1 = as_avgpool_down[_image]_f32 (res / ldr optional, lrelu = the image holds LeakyReLU(y)), 2 = as_stem_pool_image_f32 (w = the
 * stem's fp32 image [T][Kp][C], bias or NULL).  y (kinds 0, 1) and yh as there; the single entry points are this with n = 1.  A problem
 * without outputs (B, max_out or Hout 0) launches nothing and writes nothing, the image's zero column included. */
typedef struct AsDownArgs {
    int32_t kind;
    const float* x; int32_t ldx;
    const int32_t* in_off; const int32_t* in_w; int32_t Hin;
    float* y; int32_t ldy;
    const int32_t* out_off; const int32_t* out_w; int32_t Hout;
    const float* w; const float* bias;
    int32_t kh, pool_h, Kp;
    const float* res; int32_t ldr;
    int32_t B, C, max_out, lrelu;
    uint16_t* yh; int32_t n_out;
} AsDownArgs;
int as_down_multi_f32(const AsDownArgs* list_host, int n, as_stream_t stream);
/* The grid of as_down_multi_f32 for one problem, a function of host-known shapes alone (csrc/down_strips.h states the rule): the output
 * image of every (utterance, 8-channel group) is cut into *strips runs of *rows output rows (the last run: what is left), one workgroup
 * each, which walks its rows 256 outputs per trip.  kind as in AsDownArgs, max_wo = the widest utterance's output columns, groups = the
 * 8-channel groups (an image: 2 * ceil(C / 16) rounded up to a multiple of 8).  Hout = 0: no strips. */
int as_down_strip_rule(int kind, int Hout, int max_wo, int B, int groups, int32_t* strips, int32_t* rows);
int as_im2col_valid_image_f32(const float* x, int ldx, const int32_t* in_off, const int32_t* in_w, const int32_t* out_off,
                              const int32_t* out_w, int K, int stride, int lrelu, int B, int C, uint16_t* yh, as_stream_t stream);
int as_mean_pool_f32(const float* x, int ldx, const int32_t* col_off, int B, int C, int lrelu, float* y, int ldy,
                     as_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * wav -> normalised log-mel front end, test.py:40-47: torchaudio MelSpectrogram(n_mels 80, n_fft 2048,
 * win 1200, hop 300) = framing (centre, reflect padding) -> windowed DFT (a conv GEMM with the basis as weights) -> power ->
 * mel filterbank (a conv GEMM) -> (log(1e-5 + mel) + 4) / 4.
 * as_frame_signal_f32: wave = utterances back to back (wav_off int32 [B+1]); X [n_fft][N] frames, utterance b's at columns
 *   frame_off[b] .. frame_off[b+1] (1 + L_b / hop of them).  as_spec_power_f32: Y [2F][N] (real rows, then imaginary) -> P [F][N].
 * ------------------------------------------------------------------------------------------- */
int as_frame_signal_f32(const float* wave, const int32_t* wav_off, const int32_t* frame_off, int B, int max_frames, int n_fft, int hop,
                        float* X, int ldx, as_stream_t stream);
int as_spec_power_f32(const float* Y, int ldy, int F, int N, float* P, int ldp, as_stream_t stream);
int as_log_norm_f32(const float* x, int ldx, int C, int N, float eps, float mean, float std, float* y, int ldy, as_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * EMA_Predictor: what is not a GEMM in Utils/EMA/EMA_Predictor.py and its conformer blocks.
 * as_xl_attention_f32: RelativeMultiHeadAttention.forward (conformer/attention.py:77-109) on a fused [3C][N] q/k/v
 *   projection and pos [C][N] = pos_proj(PE[frame index]) per utterance; u_bias, v_bias [heads][64]; the reference's
 *   _relative_shift (:111-119) is reproduced entry for entry; inv_scale = 1/sqrt(d_model).  d_head must be 64.
 * as_glu_dwconv_bn_swish_f32: GLU -> depthwise conv1d (k odd <= 63, zero 'same' padding inside the utterance) -> BatchNorm
 *   (eval, scale/shift) -> Swish (conformer/convolution.py:140-144); a [2C][N] -> y [C][N]; w [C][k].
 * as_lstm_step0_f32: one LSTM step from the zero state for every column, both directions (EMA_Predictor.py:43,79: an
 *   nn.LSTM without batch_first fed [1, T, 256] treats the T frames as a batch of length-1 sequences); gx [8H][N] -> h [2H][N].
 * ------------------------------------------------------------------------------------------- */
int as_xl_attention_f32(const float* qkv, int ld, int C, int heads, const float* pos, int ldp, const float* u_bias,
                        const float* v_bias, float inv_scale, const int32_t* col_off, int B, int max_len, float* out, int ldo,
                        as_stream_t stream);
/* as_xl_attention_image_f32: the same attention on the matrix cores (csrc/xl_attention.hip), fed by the projection GEMMs' operand images.
 *   qkv fp32 [4C][N] (ld) and qkv_h its image (as_conv_gemm_f32 with Y and Yh): rows q + u_bias, q + v_bias, k, v -- the query weights
 *   stacked twice with the biases folded in; pos_h = the image of pos [C][N]; n_total = N (the images' column count); out fp32 [C][N]
 *   and / or out_h = the result as the operand image of the out-projection GEMM (as_split_f16x2_bytes(C, N) bytes).
 *   f16x3 products (fp32-accurate); agrees with as_xl_attention_f32 to fp32 rounding. */
int as_xl_attention_image_f32(const float* qkv, int ld, const uint16_t* qkv_h, const uint16_t* pos_h, int n_total, int C, int heads,
                              float inv_scale, const int32_t* col_off, int B, int max_len, float* out, int ldo, uint16_t* out_h,
                              as_stream_t stream);
int as_glu_dwconv_bn_swish_f32(const float* a, int lda, int C, const float* w, int k, const float* scale, const float* shift,
                               const int32_t* col_off, int B, float* y, int ldy, as_stream_t stream);
int as_lstm_step0_f32(const float* gx, int ldg, int H, int N, float* h, int ldh, as_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Windowed relative-position attention (K5) on a fused [3C][N] q/k/v projection.
 * Replaces MultiHeadAttention.attention and its skew helpers, RelTransformerEnc.py:138-233.
 * emb_rel_k / emb_rel_v: [2*window+1][C/heads] (heads share them, :113-117).
 * ------------------------------------------------------------------------------------------- */
int as_relpos_attention_f32(const float* qkv, int ld, int C, int heads, int window, const float* emb_rel_k,
                            const float* emb_rel_v, const int32_t* col_off, int B, int max_len, float* out, int ldo,
                            as_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * BiLSTM recurrence (K9).  gx_tm [N][ldg >= 8H] time-major gate pre-activations W_ih x + b_ih + b_hh
 * (forward gates 0..4H-1, reverse 4H..8H-1), whh_t [2][H][4H] = W_hh transposed; out [2H][N].
 * Replaces nn.LSTM at models.py:526,555-561 and :589-591,606-618.
 * Up to AS_MAX_LSTM_JOBS independent LSTMs of the same H over the same layout (the F0 / energy / TV
 * branches, models.py:606-618) go in one launch so their sequential recurrences overlap.
 * ------------------------------------------------------------------------------------------- */
#define AS_MAX_LSTM_JOBS 4
typedef struct BiLstmJob {
    const float* gx_tm;    /* [N][ldg] */
    const float* whh_t;    /* [2][H][4H] */
    float* out;            /* [2H][ldo] */
    int32_t ldg, ldo;
} BiLstmJob;
int as_bilstm_f32(const BiLstmJob* jobs_host, int n_jobs, const int32_t* col_off, int B, int H, as_stream_t stream);
/* H = 256: the recurrence of an utterance (or a pair) split over a cluster of four workgroups that keep W_hh in registers and exchange h
 * every step through `xchg` -- a device buffer of as_bilstm_cluster_bytes(n_jobs, B) bytes that the caller zero-fills ONCE and then leaves
 * to the library (it carries launch epochs; launches that may overlap in time need separate buffers).  max_len = longest utterance.
 * Falls back to as_bilstm_f32 when the grid would not fit the chip at once, for other H, or with xchg == NULL. */
/* A member's poll is bounded (~1 s); one that gives up raises AS_STATUS_LSTM_TIMEOUT (as_device_status above): the output is then void. */
size_t as_bilstm_cluster_bytes(int n_jobs, int B);
int as_bilstm_cluster_f32(const BiLstmJob* jobs_host, int n_jobs, const int32_t* col_off, int B, int H, int max_len, void* xchg,
                          size_t xchg_bytes, as_stream_t stream);

/* The kernel a launch takes, decided in one place (csrc/lstm_rule.h: host only, no device needed; the same header gives the launch's
 * geometry and the cluster kernels' id, word and tag arithmetic): what as_bilstm_f32 (has_xchg = 0) and
 * as_bilstm_cluster_f32 (has_xchg = xchg != NULL) run for these arguments, or AS_EINVAL for an n_jobs / B / H they refuse.
 *   QUAD1    H = 64 / 128, one utterance per workgroup, while n_jobs * 2 * B <= 512
 *   QUAD     H = 16 / 32 / 64 / 128, two utterances per workgroup
 *   BIG      H = 256 in one workgroup;  STREAM  every other H divisible by 16 (W_hh streamed from L2)
 *   CLUSTER1 / CLUSTER2  H = 256 over clusters of four workgroups, one / two utterances per cluster: needs the exchange buffer
 *            (xchg_bytes >= as_bilstm_cluster_bytes), 0 < max_len < 2^17 and at most 64 clusters; AS_LSTM_CLUSTER in the environment
 *            ("0" / "1" / "2") overrides the choice between never / one / two. */
enum { AS_LSTM_PLAN_QUAD1 = 0, AS_LSTM_PLAN_QUAD = 1, AS_LSTM_PLAN_BIG = 2, AS_LSTM_PLAN_STREAM = 3, AS_LSTM_PLAN_CLUSTER1 = 4,
       AS_LSTM_PLAN_CLUSTER2 = 5 };
int as_bilstm_plan(int n_jobs, int B, int H, int max_len, int has_xchg, size_t xchg_bytes);

/* test hooks: member `drop_member` (0..3; -1 = none) of every cluster exits at once and a poll gives up after spin_limit tries
 * (0 = default), so that the failure path can be exercised in milliseconds */
int as_bilstm_cluster_test_hooks(int drop_member, int spin_limit);

/* ---------------------------------------------------------------------------------------------
 * HiFi-GAN generator glue (Vocoder/vocoder.py:75-125).  Its convolutions run through
 * as_conv_gemm_f32 (dilated taps, LeakyReLU slopes 0.1 / 0.01, tanh epilogue).
 * ------------------------------------------------------------------------------------------- */
/* ConvTranspose1d(k = 2u, stride u) = one 3-tap conv with output rows (phase r, channel m), then
 * y[m][u*q + r] = z[r*C + m][q] + bias[m]                                     vocoder.py:84-89,102-103 */
int as_interleave_phases_f32(const float* z, int ldz, const float* bias, int C, int u, int Nin, float* y, int ldy,
                             as_stream_t stream);
/* y = (a + b + c) / 3 over [C][N]                                              vocoder.py:104-110 */
int as_mean3_f32(const float* a, const float* b, const float* c, int ld, int C, int N, float* y, int ldy, as_stream_t stream);
/* LeakyReLU((a + b + c) / 3, slope) as the split operand image (as_split_f16x2_bytes(C, N) bytes) of the conv that follows -- the next
 * stage's ConvTranspose1d (vocoder.py:101-110): the fp32 mean is read by nothing else. */
int as_mean3_image_f32(const float* a, const float* b, const float* c, int ld, int C, int N, float slope, uint16_t* xh, as_stream_t stream);
/* conv_post (vocoder.py:97, 111-113): y [N] = act(conv1d(LeakyReLU(x [C][N], in_slope), w fp32 [C][k]) + bias[0]) with ONE output channel,
 * zero padding per utterance (meta = the layout's column descriptors), act = tanh when tanh_out; k = 3, 5 or 7.  Plain fp32 FMAs: a read of x. */
int as_conv_post_f32(const float* x, int ldx, int C, int N, const float* w, const float* bias, int k, float in_slope, int tanh_out,
                     const uint64_t* meta, float* y, as_stream_t stream);
/* as_conv_post_f32 with the samples (also, or with y NULL: only) as 16-bit PCM, written by the same pass -- the waveform is never re-read:
 *     pcm = (int16) fmaxf(-32768.f, fminf(32767.f, rintf(32767.f * w)))        w = the fp32 sample y would get
 * (one fp32 multiply, round half to even, saturate).  A NaN sample stores 0 and raises AS_STATUS_F16_RANGE; the fp32 output is as
 * as_conv_post_f32 writes it.  At least one of y and pcm; pcm 2-byte aligned (4-byte aligned: two samples per store). */
int as_conv_post_pcm_f32(const float* x, int ldx, int C, int N, const float* w, const float* bias, int k, float in_slope, int tanh_out,
                         const uint64_t* meta, float* y, int16_t* pcm, as_stream_t stream);
/* One residual step of ResBlock1 (vocoder.py:35-42) as ONE launch, for the stages with C = 32 or 64 channels:
 *     y = x + conv2(lrelu(conv1(lrelu(x))))        conv1: k taps with dilation dil, conv2: k taps with dilation 1, zero padding per utterance
 * x, y fp32 [C][N] (y != x: a workgroup reads its neighbours' columns of x); w1, w2 = the conv GEMM's weight images of the two
 * [C][C][k] weights (as_prep_weight_f16x2_host, G = 1), scale1 / scale2 = 1 / their scales, b1 / b2 [C] or NULL; slope = LeakyReLU's;
 * col_off int32 [B + 1] = the utterances' first columns (packed frames), max_w = the widest utterance; k odd <= 17, dil * (k / 2) <= 40.
 * add1 / add2 (both or neither; [C][N], ld_add): y = ((add1 + add2) + y) / out_div -- the mean of the three stacks of a stage
 * (vocoder.py:104-110) folded into the last step of the third.  yh: the result also (or, with y NULL, only) as the split operand image
 * of the next conv (as_split_f16x2_bytes(C, N) bytes; LeakyReLU(yh_slope) applied first).  Same f16x3 arithmetic as as_conv_gemm_f32; the tile's columns stay in
 * LDS between the two convs (csrc/respair.hip). */
typedef struct AsResPairArgs {
    const float* x; int32_t ldx;
    float* y; int32_t ldy;
    const uint16_t* w1; const uint16_t* w2;
    const float* b1; const float* b2;
    float scale1, scale2;
    int32_t C, N, k, dil;
    float slope;
    const int32_t* col_off; int32_t B, max_w;
    const float* add1; const float* add2; int32_t ld_add; float out_div;
    uint16_t* yh; float yh_slope;       /* optional: LeakyReLU(y, yh_slope) as the operand image of the conv that follows (y may then be NULL) */
    int32_t x_u; const float* x_bias;   /* x_u >= 2: x is the phase-major ConvTranspose1d output z [x_u * C][N / x_u] (ldx its row stride) and
                                         * x[ch][col] = z[(col % x_u) * C + ch][col / x_u] + x_bias[ch]: as_interleave_phases_f32 folded into the read */
} AsResPairArgs;
int as_respair_f32(const AsResPairArgs* a, as_stream_t stream);
/* The glue kernels under a capacity layout (as_vocoder_forward_cap): N is room, *n_valid (a DEVICE int; NULL = N: exactly the functions
 * above) the leading columns that hold utterances.  Filler columns are neither read nor written -- except by conv_post, the last kernel,
 * which stores 0 for them (y and pcm in [*n_valid, N)): a NaN in uninitialised filler reaches no result and raises nothing.
 * as_interleave_phases_cap_f32 counts INPUT columns (of Nin). */
int as_interleave_phases_cap_f32(const float* z, int ldz, const float* bias, int C, int u, int Nin, const int32_t* n_valid, float* y, int ldy,
                                 as_stream_t stream);
int as_mean3_cap_f32(const float* a, const float* b, const float* c, int ld, int C, int N, const int32_t* n_valid, float* y, int ldy,
                     as_stream_t stream);
int as_mean3_image_cap_f32(const float* a, const float* b, const float* c, int ld, int C, int N, const int32_t* n_valid, float slope,
                           uint16_t* xh, as_stream_t stream);
int as_conv_post_pcm_cap_f32(const float* x, int ldx, int C, int N, const float* w, const float* bias, int k, float in_slope, int tanh_out,
                             const uint64_t* meta, const int32_t* n_valid, float* y, int16_t* pcm, as_stream_t stream);
/* The generator's geometry tables from DEVICE offsets, one launch (csrc/vocoder.hip; what as_vocoder_forward_cap runs first).
 * off int32 [B + 1] (off[0] = 0, ascending) counts units of `mult` mel frames; cap = mel frames of room for all utterances together;
 * max_len = the mel frames one utterance may have (0 = cap); rates_host [n_rates <= 9] = columns per mel frame of every layout (1, then
 * the running products of the upsample rates: 1, 10, 50, 150, 300).  With o_b = min(off[b] * mult, cap), rate r writes
 *     tab  int32 [n_rates][2 B + 2]:  w[b] = r (o_{b+1} - o_b),  off_r[b] = r o_b (B + 1 entries),  n_valid = r o_B
 *     meta uint64 [cap * sum r]:      rate i's table starts at cap * (r_0 + ... + r_{i-1}); column off_r[b] + j = AS_META_PACK(0, j, 1, w[b]);
 *                                     the descriptors of the filler [n_valid, r cap) are left alone
 * and sample_off (optional, [B + 1]) = off_r of the last rate.  off[B] * mult > cap or an utterance of more than max_len frames raises
 * AS_STATUS_CAPACITY (the layout is cut at cap: nothing is written past it); w[b] > AS_META_MAX_W raises AS_STATUS_BAD_LAYOUT and that
 * utterance's columns get AS_META_PACK(0, 0, 1, 1).  AS_EINVAL: B < 1, mult < 1, cap < 1, max_len > cap, r cap >= 2^31. */
int as_vocoder_cap_geometry(const int32_t* off, int B, int mult, int cap, int max_len, int n_rates, const int32_t* rates_host, int32_t* tab,
                            uint64_t* meta, int32_t* sample_off, as_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Module-level entry points: the acoustic model behind an opaque handle.  A C / C++ host runs
 * the whole path of models.py:356-371 -- ArtsSpeech.forward(step="test") -- or one sub-module at a time through these; the
 * Python mirror of the reference's classes (artspeech_amd/models.py) is a thin caller of the same functions.
 *
 * as_model  = the weights: immutable after as_model_create, shareable between host threads, one per GPU.
 *             Exception to the conventions above: as_model_create ALLOCATES device memory (the prepared weights,
 *             ~1.3 GB for the shipped configuration) on the current HIP device and synchronises; as_model_destroy frees it.
 * as_plan   = per-caller mutable state: the small device tables of the batch geometries it has seen (utterance offsets,
 *             column descriptors), side HIP streams and events for the independent branches.  Not thread-safe: one per
 *             host thread / stream.  The first call with a new geometry uploads its tables and synchronises the stream
 *             (do not capture that call into a hipGraph); later calls with the same geometry only enqueue kernels.
 * All activations are "packed frames" (above): every utterance of the batch back to back along the column axis, no padding.
 * Workspaces are caller-owned device memory (256-byte aligned); as_module_workspace_bytes says how much a call needs.
 * ------------------------------------------------------------------------------------------- */
typedef struct as_model as_model;
typedef struct as_plan as_plan;
#define AS_ENOSPC (-2)      /* an output buffer or workspace is too small */

/* models.py:680-683 build_model(args): the Munch fields the inference path reads (config.yml model_params), plus the
 * normalisation statistics of Data/stats.json that StyleEncoder.forward applies (models.py:447-449; utils.py:86-92). */
typedef struct as_model_cfg {
    int32_t hidden_dim;    /* 512: channels of the encoders / predictors / decoder */
    int32_t dim_in;        /* 64: first width of the style towers */
    int32_t style_dim;     /* 256 (the Style vector has 2 * style_dim entries; its slices are hard-coded, models.py:499,597-599) */
    int32_t n_mels;        /* 80 */
    int32_t n_token;       /* 178 */
    int32_t reserved;
    float stats[24];       /* energy_mean, energy_std, pitch_mean, pitch_std, EMA_mean[10], EMA_std[10] */
} as_model_cfg;

/* blob_host: the checkpoint's ArtsSpeech state_dict in the reference's own key layout (weight_norm g / v, spectral_norm
 * orig / u / v) serialised as
 *     "ASWBLOB1" | u32 n | n x { u16 name_len | name | u8 ndim | u32 dims[ndim] | u64 data_offset } | u64 data_bytes | fp32 data
 * (little endian; data_offset counts from the start of the data section; artspeech_amd/blob.py writes it from a
 * state_dict).  Folds weight_norm / spectral_norm (models.py:685-701 does it implicitly on every forward), lays every
 * weight out for the kernels and uploads it. */
int as_model_create(const void* blob_host, size_t blob_bytes, const as_model_cfg* cfg, as_model** out);
int as_model_destroy(as_model* m);
/* the configuration the model was created with */
int as_model_get_cfg(const as_model* m, as_model_cfg* out);
int as_plan_create(const as_model* m, as_plan** out);
int as_plan_destroy(as_plan* p);
/* on = 1: the independent branches of a forward run on the calling stream instead of on side streams (one chain per batch: the
 * arrangement as_lanes keeps several of in flight).  as_plan_set_merge (default on; it matters for serial plans only): the branches'
 * launches are recorded first and played out in an order that lets conv GEMMs of independent branches -- the towers, the triple encoder,
 * dur_block and the duration predictor's blocks: models.py:356-360, 417-424, 540-546 have no edge between them -- share launches
 * (as_conv_gemm_multi_f32): on one stream a step costs the sum of its kernels' durations, and a small conv beside a large one costs next to
 * nothing.  off: every branch whole, one after the other, one launch per conv.  Set both before asking for workspace sizes and do not
 * change them between as_forward_test_begin and _finish (the order of the workspace allocations follows the flags). */
int as_plan_set_serial(as_plan* p, int on);
int as_plan_set_merge(as_plan* p, int on);
/* on = 1: as_forward_test records phase marks (HIP events) on the calling stream; as_plan_phase_ms then returns the ms of the
 * last call's phases: [0] reference features + tower inputs, [1] the concurrent branches (encoders, towers, duration predictor),
 * [2] durations + AdaIN fc + articulatory predictors, [3] decoder.  Blocks until that call has finished. */
int as_plan_set_timing(as_plan* p, int on);
/* matrix-core products per fp32 product in this plan's forwards: 3 = f16x3 (fp32-accurate, default); 1 = plain fp16 operands
 * (the 16-bit-operand mode BASELINE.md names for config C2; its error is reported by bench.py and tests/test_net_gpu.py) */
int as_plan_set_operand_mode(as_plan* p, int n_prod);
/* Per-token prosody: control INSIDE an utterance (stress a word, lengthen a pause, raise the pitch towards the end of a question, open the
 * jaw on one vowel), as state of the plan.  Row i belongs to packed token i (the order of as_forward_io.tokens) and has the columns of a
 * prosody row (AS_PROSODY_DUR, AS_PROSODY_GAIN + c, AS_PROSODY_OFFSET + c; below, next to as_forward_io.prosody).  DEVICE memory, fp32
 * [sum tok_lens][ld >= AS_PROSODY_DIM], read when a forward RUNS (a replayed graph sees new contents).
 *   Durations: token i of utterance b gets clamp(rint(v), 1, 16384) frames, v = fp32(duration[i] * rows[i][AS_PROSODY_DUR]) and then, with
 *   as_forward_io.prosody set too, v = fp32(v * prosody[b][AS_PROSODY_DUR]); `duration` stays the unscaled predictor output, dur_i,
 *   frame_off and everything behind them follow the controlled counts (known frames: batch->frames must be their sums).  A pause is a
 *   scale on a space or punctuation token.
 *   Tracks: token k of an utterance covers the full-rate columns [S_k, S_k + 2 d_k) (S_k = twice the frames before it) and has its centre at
 *   S_k + d_k; column j has the midpoint j + 0.5.  smooth 0: a token's gains / offsets hold over its columns.  smooth 1: they are control
 *   points at the tokens' centres, joined linearly inside an utterance (never across utterances), constant before the first and after the
 *   last centre: between the centres c_k < j + 0.5 < c_{k+1}, w = fp32((j + 0.5 - c_k) / (c_{k+1} - c_k)) and q(j) = fmaf(w, q_{k+1} - q_k,
 *   q_k) for each of the 24 parameters q.  Every track value x of the column (after the utterance's own gain and offset, if any) becomes
 *   fmaf(gain(j), x, offset(j)) before the decoder or the F0 / N / EMA outputs read it.  Filler columns of a capacity layout are not touched.
 *   Identity rows {1, 1 x 12, 0 x 12} give the results of a plan without controls bit for bit, in either mode (a -0 track value may come
 *   back as +0).
 * The struct is copied; tp NULL = off (the default): a forward then issues exactly the launches it issued before this entry point existed.
 * With controls set a forward adds three small launches (csrc/token_prosody.hip) and two small buffers, which both halves keep in
 * workspace A (workspace B is laid out as without controls): set them BEFORE asking as_module_workspace_bytes (AS_MOD_FORWARD_A /
 * _A_VOICE / _B / _B_CAP then count a call with controls), like as_plan_set_serial, and do not change them between
 * as_forward_test_begin and _finish.  Works with known frames, the read-back, frame_cap (no synchronisation, no host read, no
 * allocation: capturable), voice mode and together with as_forward_io.prosody.  AS_EINVAL: p NULL, rows NULL, ld < AS_PROSODY_DIM, smooth
 * not 0 or 1; and from as_forward_test / _begin / _finish on a plan with controls set when io->forced_dur (forced durations would ignore the
 * scales) or io->segs is given -- before anything is launched.  as_lanes never sets them on its plans. */
typedef struct as_token_prosody { const float* rows; int32_t ld; int32_t smooth; } as_token_prosody;
int as_plan_set_token_prosody(as_plan* p, const as_token_prosody* tp);   /* copied; NULL = off (the default) */
/* Fit to time: spans of tokens spoken in an exact number of frames ("say this in 2.40 s", "this word ends at 1.2 s"), as state of the plan.
 * Span s = the packed tokens [span_tok[s][0], + span_tok[s][1]) of ONE utterance, in ascending order without overlap; span_frames[s] = its
 * target in half-rate frames (one = 2 mel frames = 25 ms at 24 kHz).  When a forward runs, the tokens of a span get integer durations that
 * add up to the target exactly, lie in [1, 16384] and stay proportional to the controlled durations v (the predictor's values under
 * as_forward_io.prosody and the per-token duration scales): the rule, its bounds and why the pinned tokens are a prefix are in
 * csrc/duration_fit.h.  Tokens outside every span are rounded as without a fit; lock[i] != 0 keeps token i's own rounded duration and lets
 * the rest of its span absorb the difference (hold the pauses and stretch the speech, or the reverse).
 *   A structural defect (first < 0, count < 1, first + count past the tokens, spans out of order or overlapping) voids the whole fit; a span
 *   with count > max_count, across an utterance boundary, with a target its free tokens cannot meet inside [1, 16384] each (or, with no free
 *   token, other than the locked sum) voids that span.  Void tokens get the plain rounding and AS_STATUS_BAD_LAYOUT is raised.
 * All three arrays are DEVICE memory read when the call RUNS: a replayed graph sees new targets.  dur_i, frame_off, the frame -> token map,
 * the marks and everything behind them follow the fitted counts (known frames: batch->frames must be their sums -- with every utterance
 * covered by spans the host knows them before the call).
 * as_plan_set_fit       the struct is copied; fit NULL = off (the default): a forward then issues exactly the launches and needs exactly
 *                       the workspace it did before this entry point existed.  With a fit a forward adds two small launches
 *                       (csrc/duration_fit.hip) and two small buffers in workspace A (workspace B is laid out as without): set it BEFORE
 *                       asking as_module_workspace_bytes, and do not change it between as_forward_test_begin and _finish.  Works with known
 *                       frames, the read-back, frame_cap (capturable), voice mode, as_forward_io.prosody and per-token prosody.
 *                       AS_EINVAL: p NULL, a NULL span_tok / span_frames, n_spans or max_count outside [1, 4096]; and from
 *                       as_forward_test / _begin / _finish on a plan with a fit when io->forced_dur or io->segs is given -- before anything
 *                       is launched.  as_lanes never sets one on its plans.
 * as_fit_durations_f32  the kernels on their own: v [n_tokens] (DEVICE, already controlled) -> dur_i [n_tokens] for EVERY token, and
 *                       (optional) span_scale_q16 [n_spans] = floor(R * 65536 / U*), the stretch the span received in units of 2^-16 (0 for
 *                       a void span or one without a free token), so that a caller can refuse an unnatural fit.  Two launches; nothing is
 *                       read back, uploaded, allocated or waited for: capturable.  A non-finite v raises AS_STATUS_F16_RANGE (its plain
 *                       duration is 1, its weight that of 1).  AS_EINVAL: NULL v / tok_off / fit / dur_i / ws, B outside [1, 1024],
 *                       n_tokens < 0, the fit as above; AS_ENOSPC: ws_bytes below as_fit_workspace_bytes(n_tokens, fit) (0 for arguments it
 *                       refuses); AS_EDEVICE while a status bit is set.
 * as_fit_host           the same rule on HOST arrays (every pointer, those of fit included, is a host pointer; no GPU, no workspace);
 *                       AS_EDEVICE where the device would raise a status. */
typedef struct as_fit {
    const int32_t* span_tok;     /* DEVICE [n_spans][2]: first packed token, count */
    const int32_t* span_frames;  /* DEVICE [n_spans]: target, half-rate frames; read when the call RUNS */
    const int32_t* lock;         /* DEVICE [sum tok_lens] or NULL */
    int32_t n_spans;             /* 1 .. 4096 */
    int32_t max_count;           /* 1 .. 4096: sizes the launch */
} as_fit;
int as_plan_set_fit(as_plan* p, const as_fit* fit);   /* copied; NULL = off (the default) */
size_t as_fit_workspace_bytes(int n_tokens, const as_fit* fit);
int as_fit_durations_f32(const float* v, const int32_t* tok_off, int B, int n_tokens, const as_fit* fit, int32_t* dur_i,
                         int32_t* span_scale_q16, void* ws, size_t ws_bytes, as_stream_t stream);
int as_fit_host(const float* v, const int32_t* tok_off, int B, int n_tokens, const as_fit* fit, int32_t* dur_i, int32_t* span_scale_q16);
int as_plan_phase_ms(as_plan* p, float* ms, int n);
/* The plan caches the device tables of every batch geometry it has seen (key: the whole length vector).  Above max_layouts entries
 * (default 4096, minimum 64) the next entry point first waits for the streams THIS plan has launched on (not for the device: other plans'
 * work goes on), drops the cache and reuses its table memory: memory stays bounded under ever new ragged batches.  The flush never runs
 * while the calling stream is being captured (it then waits for the next entry point).  A hipGraph captured from a plan holds table
 * addresses -- give captured geometries a plan of their own whose cap is never reached, and reset it (as_plan_reset_layouts) only
 * together with its graphs: as_lanes does.  as_plan_layout_flushes: how often the cache has been dropped; as_plan_layout_count: entries
 * held now.  as_plan_reset_layouts: drop the cache now -- the caller guarantees that no work launched from this plan is in flight and that
 * no graph captured from it will be launched again. */
int as_plan_set_layout_cap(as_plan* p, int max_layouts);
int as_plan_layout_flushes(const as_plan* p);
int as_plan_layout_count(const as_plan* p);
int as_plan_reset_layouts(as_plan* p);

/* geometry of one batch: HOST arrays */
typedef struct as_batch {
    int32_t B;
    const int32_t* tok_lens;   /* [B] tokens per utterance (text modules) */
    const int32_t* ref_lens;   /* [B] reference mel frames per utterance (style modules) */
    const int32_t* frames;     /* [B] half-rate frames per utterance = sum of its integer durations (predictors / decoder);
                                  as_forward_test: NULL = not known yet, read back from the device (one stream synchronisation) */
} as_batch;

enum { AS_MOD_FORWARD_A = 0, AS_MOD_FORWARD_B = 1, AS_MOD_ENCODER = 2, AS_MOD_STYLE = 3, AS_MOD_DURATION = 4, AS_MOD_ARTS = 5,
       AS_MOD_DECODER = 6, AS_MOD_FORWARD_B_CAP = 7, AS_MOD_VOICE = 8, AS_MOD_FORWARD_A_VOICE = 9 };
/* workspace bytes of one module call for this geometry (AS_MOD_FORWARD_A / _B: the two workspaces of as_forward_test; AS_MOD_FORWARD_B_CAP:
 * workspace B of a call with as_forward_io.frame_cap = the SUM of batch->frames, whose entries are then capacities, not counts;
 * AS_MOD_VOICE: as_voice_forward; AS_MOD_FORWARD_A_VOICE: workspace A of a voice-mode forward (as_forward_io.voices), batch->ref_lens is not
 * read.  Workspace B of a voice-mode forward is AS_MOD_FORWARD_B / _B_CAP; with batch->ref_lens NULL they are counted for voice mode) */
size_t as_module_workspace_bytes(const as_model* m, as_plan* p, int module, const as_batch* batch);

/* RelTransformerEncoder.forward (RelTransformerEnc.py:371-380).  which: 0 text_encoder, 1 arts_encoder, 2 the duration
 * predictor's text_encoder.  tokens int32 [sum tok_lens]; out fp32 [hidden_dim][ldo >= sum tok_lens] (the reference returns
 * its transpose, padded per utterance). */
int as_encoder_forward(const as_model* m, as_plan* p, int which, const as_batch* batch, const int32_t* tokens, float* out, int ldo,
                       void* ws, size_t ws_bytes, as_stream_t stream);
/* StyleEncoder.forward (models.py:426-472) behind the two frozen extractors: mel [n_mels][ldm], f0_raw [sum ref_lens],
 * ema_raw [10][lde] (models.py:432-433 outputs) -> feat12 [12][ldf] (row 0 energy n_ext, 1 f0_ext, 2..11 ema_ext, normalised),
 * style [B][2 * style_dim]. */
int as_style_forward(const as_model* m, as_plan* p, const as_batch* batch, const float* mel, int ldm, const float* f0_raw,
                     const float* ema_raw, int lde, float* feat12, int ldf, float* style, void* ws, size_t ws_bytes, as_stream_t stream);
/* DurationPredictor.forward (models.py:540-566): tokens, ema_ext [10][lde] (rows 2..11 of feat12) -> duration fp32 [sum tok_lens] */
int as_duration_forward(const as_model* m, as_plan* p, const as_batch* batch, const int32_t* tokens, const float* ema_ext, int lde,
                        float* duration, void* ws, size_t ws_bytes, as_stream_t stream);
/* ArtsPredictor.forward (models.py:596-621): a_ens [hidden_dim][lda >= sum frames], style [B][2 * style_dim] ->
 * F0, N [1][ldp], EMA [10][ldp], ldp >= 2 * sum frames */
int as_arts_forward(const as_model* m, as_plan* p, const as_batch* batch, const float* a_ens, int lda, const float* style, float* F0,
                    float* N, float* EMA, int ldp, void* ws, size_t ws_bytes, as_stream_t stream);
/* Decoder.forward (models.py:497-517): asr [hidden_dim][lda >= sum frames] (half rate; the x2 nearest up-sampling of
 * models.py:500 happens inside), style, F0 / N [1][ldp], EMA [10][ldp] -> mel [n_mels][ldo >= 2 * sum frames] */
int as_decoder_forward(const as_model* m, as_plan* p, const as_batch* batch, const float* asr, int lda, const float* style,
                       const float* F0, const float* N, const float* EMA, int ldp, float* mel, int ldo, void* ws, size_t ws_bytes,
                       as_stream_t stream);

/* Voices: everything forward(step="test") takes from the reference utterance reduces to two vectors per speaker -- Style [2 * style_dim]
 * (StyleEncoder.style_extractor on the T - 1 crop of the reference features, models.py:459-471; slices timbre [0, style_dim), TV
 * [style_dim, 3/2 style_dim), F0 and energy the two quarters behind) and dur_style [style_dim / 4] (dur_linear(dur_block(ema_ext)) on the
 * full-length TV track, models.py:541-546).  A voice is the two back to back: as_voice_dim(m) = 2 * style_dim + style_dim / 4 fp32,
 * [0, 2 style_dim) Style, then dur_style.  as_voice_forward computes the voices of B reference utterances (batch->ref_lens; mel / f0_raw /
 * ema_raw as in as_forward_io) into rows of voice [B][ld_voice >= as_voice_dim] (workspace: AS_MOD_VOICE) -- the same quantities the full
 * forward computes -- and a forward with as_forward_io.voices set reads them instead of the reference: the style towers, the reference
 * features and dur_block do not run at all. */
int as_voice_dim(const as_model* m);
int as_voice_forward(const as_model* m, as_plan* p, const as_batch* batch, const float* mel, int ldm, const float* f0_raw, const float* ema_raw,
                     int lde, float* voice, int ld_voice, void* ws, size_t ws_bytes, as_stream_t stream);

/* ArtsSpeech.forward(step="test") (models.py:356-371), batched: every utterance gets exactly its batch-1 result.
 * Two halves sharing workspace A: _begin runs everything up to the integer durations (encoders, style towers, duration
 * predictor; results stay in ws_a), _finish the alignment expansion, the articulatory predictors and the decoder (needs
 * batch->frames).  as_forward_test = both; with batch->frames == NULL it synchronises the stream once in between to read the
 * frame counts (returns AS_ENOSPC if ld_out or ws_b turn out too small; frames_host_out, if given, then says what is needed). */
typedef struct as_forward_io {
    /* inputs (device) */
    const int32_t* tokens;               /* [sum tok_lens] */
    const float* mel; int32_t ld_mel;    /* [n_mels][ld_mel >= sum ref_lens] normalised log-mel of the reference utterances */
    const float* f0_raw;                 /* [sum ref_lens]      pitch extractor output (models.py:432) */
    const float* ema_raw; int32_t ld_ema;/* [10][ld_ema]        EMA extractor output (models.py:433) */
    const int32_t* forced_dur;           /* optional [sum tok_lens]: integer durations replacing the predictor's (benchmarks) */
    /* output (device) */
    float* mel_out; int32_t ld_out;      /* [n_mels][ld_out >= 2 * sum frames] */
    /* optional outputs (device; NULL = not wanted) */
    float* duration;                     /* [sum tok_lens] fp32 durations before rounding */
    int32_t* dur_i;                      /* [sum tok_lens] integer durations (round half even, clamp >= 1) */
    int32_t* frame_off;                  /* [B + 1] half-rate frame offsets */
    float* style;                        /* [B][2 * style_dim] */
    float* feat12; int32_t ld_feat;      /* [12][ld_feat >= sum ref_lens] */
    float* t_en; float* a_en; int32_t ld_en;          /* [hidden_dim][ld_en >= sum tok_lens] */
    float* F0; float* N; float* EMA; int32_t ld_pred; /* [1] / [1] / [10] x [ld_pred >= 2 * sum frames] */
    /* Predicted durations WITHOUT the host read-back (batch->frames == NULL and frame_cap > 0).  models.py:361-368 sizes the second half
     * from the durations the first half predicts; frame_cap = the half-rate frames the caller makes ROOM for, all utterances together
     * (ld_out >= 2 * frame_cap, ld_pred likewise; the workspace of AS_MOD_FORWARD_B_CAP).  Every launch of the second half is then sized by
     * the capacity, the utterances' real extents are derived on the device (frame_off, optional output here, tells the caller where each
     * utterance's frames lie: utterance b at columns [2 frame_off[b], 2 frame_off[b + 1]) of mel_out), columns behind them are filler that
     * costs next to nothing (ConvGemmArgs.n_valid) -- and the call neither synchronises nor depends on values the host does not have: it
     * can be captured into a hipGraph, and as_lanes replays and coalesces it.  More frames than room: AS_STATUS_CAPACITY (what was computed
     * was cut at the capacity; nothing is written out of bounds; run again with more room).  frames_host_out is not written.
     * Optional outputs in this mode: frame_off, dur_i, duration, style, feat12, t_en, a_en, F0 / N / EMA. */
    int32_t frame_cap;
    /* a merged call (as_lanes coalescing under frame_cap): the submissions it was made of.  Utterances [first[s], first[s + 1]) came with
     * submission s, whose own output buffer mel_out[s] (row stride ld_out[s] >= 2 cap[s]) gets its utterances from its first column on and
     * whose frame_off[s] (optional, [its utterances + 1]) counts from 0 -- every submission is served as if it had been alone.  NULL: the
     * call is one submission (mel_out / frame_off above). */
    const struct as_segments* segs;
    /* Voice mode (voices != NULL): utterance b speaks in row voice_idx[b] of the DEVICE table voices [n_voices][ld_voice >= as_voice_dim]
     * (as_voice_forward's rows); voice_idx DEVICE int32 [B], read when the call runs (a replayed graph sees new contents), or NULL = row b.
     * mel, f0_raw, ema_raw and batch->ref_lens are not read (they may be NULL); feat12 cannot be asked for (AS_EINVAL); `style` gets the
     * gathered rows.  An index outside [0, n_voices) raises AS_STATUS_BAD_VOICE (that utterance gets a zero voice; nothing is read out of
     * bounds).  Workspace A: AS_MOD_FORWARD_A_VOICE.  Works with known frames, the read-back, frame_cap and as_forward_test_begin / _finish. */
    const float* voices; int32_t ld_voice; int32_t n_voices;
    const int32_t* voice_idx;
    /* Prosody control (prosody != NULL): how each utterance is spoken.  DEVICE fp32 [B][ld_prosody >= AS_PROSODY_DIM], read when the call
     * runs (a replayed graph sees new contents).  Row b: [AS_PROSODY_DUR] dur_scale, then for the twelve tracks the articulatory predictors
     * hand the decoder (F0, N, EMA0..9, normalised by the model's stats, as_model_cfg.stats) a gain [AS_PROSODY_GAIN + c] and an offset
     * [AS_PROSODY_OFFSET + c].  Utterance b's integer durations are clamp(rint(duration * dur_scale), 1, 16384) (one fp32 multiply; `duration`
     * stays the unscaled predictor output; dur_i, frame_off and everything behind them follow the scaled counts -- with known frames,
     * batch->frames must be their sums), and every track value x of its frames becomes fmaf(gain, x, offset) before the decoder or the
     * F0 / N / EMA outputs read it.  The identity row {1, 1 x 12, 0 x 12} gives the results of prosody == NULL bit for bit (a -0 track
     * value may come back as +0).  AS_EINVAL for ld_prosody < AS_PROSODY_DIM and together with forced_dur.  Works with known frames, the
     * read-back, frame_cap, as_forward_test_begin / _finish, voice mode and merged calls; it adds no launch.
     * Control INSIDE an utterance -- one such row per token -- is state of the plan: as_plan_set_token_prosody (above); the two compose. */
    const float* prosody; int32_t ld_prosody;
} as_forward_io;
#define AS_PROSODY_DIM 25
#define AS_PROSODY_TRACKS 12
#define AS_PROSODY_DUR 0
#define AS_PROSODY_GAIN 1
#define AS_PROSODY_OFFSET 13
typedef struct as_segments {
    int32_t n;                      /* 1 .. AS_MAX_SEGMENTS */
    int32_t first[17];
    int32_t cap[16];                /* half-rate frames of room of submission s; their sum = frame_cap */
    float* mel_out[16]; int32_t ld_out[16];
    int32_t* frame_off[16];
} as_segments;
#define AS_MAX_SEGMENTS 16
int as_forward_test_begin(const as_model* m, as_plan* p, const as_batch* batch, const as_forward_io* io, void* ws_a, size_t ws_a_bytes,
                          as_stream_t stream);
int as_forward_test_finish(const as_model* m, as_plan* p, const as_batch* batch, const as_forward_io* io, void* ws_a, size_t ws_a_bytes,
                           void* ws_b, size_t ws_b_bytes, as_stream_t stream);
int as_forward_test(const as_model* m, as_plan* p, const as_batch* batch, const as_forward_io* io, void* ws_a, size_t ws_a_bytes,
                    void* ws_b, size_t ws_b_bytes, int32_t* frames_host_out, as_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The HiFi-GAN generator behind an opaque handle (csrc/vocoder_rt.hip; Vocoder/vocoder.py:75-125, test.py:115): mel in, samples out,
 * ONE call -- the launch sequence artspeech_amd/vocoder.py issues operator by operator, in the library.
 *
 * as_vocoder = the generator's weights: immutable after as_vocoder_create, shareable between host threads, one per GPU (like as_model:
 *              as_vocoder_create ALLOCATES device memory on the current HIP device and synchronises; as_vocoder_destroy frees it).
 * blob_host  = the Generator's state dict in the "ASWBLOB1" format of as_model_create: conv_pre / ups.i / resblocks.n.convs1|2.j /
 *              conv_post, each as weight_g + weight_v + bias (weight_norm, folded here) or as weight + bias (a checkpoint saved after
 *              remove_weight_norm()).  The ConvTranspose1d -> 3-tap phase conv rewrite (as_vocoder_fold_upsample_host), the per-row
 *              biases, the fp32 conv_post row and the weight images are made here.
 * as_plan    = the per-caller cache of geometry tables, as for the acoustic model (layouts at 1x and at every stage's rate of `lens`).
 *              as_vocoder_plan_create makes one that needs no as_model: freed by as_plan_destroy, it serves as_vocoder_* only; a plan made
 *              by as_plan_create serves too.  The first call with a new geometry uploads tables and synchronises the stream (do not
 *              capture it); later calls with that geometry only enqueue kernels on `stream`, take nothing from the host but the
 *              arguments and allocate nothing: they can be captured into a hipGraph.  The chain is serial: no side streams.
 * AS_EINVAL: k != 2 u, u < 2, channels that do not halve n_stages times, n_stacks != 3 (ResBlock1 of Vocoder/config.json), a tensor
 * missing from the blob or of another shape, B < 1, a negative length, an utterance of more than AS_META_MAX_W samples, both outputs
 * NULL, ld_mel < sum lens; AS_ENOSPC: workspace too small (nothing is launched); AS_EDEVICE while a device status bit is set.
 * ------------------------------------------------------------------------------------------- */
typedef struct as_vocoder as_vocoder;
typedef struct as_vocoder_cfg {                 /* Vocoder/config.json; ResBlock1 only */
    int32_t num_mels, upsample_initial_channel;
    int32_t n_stages;  int32_t upsample_rates[8], upsample_kernel_sizes[8];      /* k == 2 u required */
    int32_t n_stacks;  int32_t resblock_kernel_sizes[4], resblock_dilations[4][4], n_dilations;   /* 3 stacks x 3 steps in config.json */
} as_vocoder_cfg;
int as_vocoder_create(const void* blob_host, size_t blob_bytes, const as_vocoder_cfg* cfg, as_vocoder** out);
int as_vocoder_destroy(as_vocoder* v);
int as_vocoder_get_cfg(const as_vocoder* v, as_vocoder_cfg* out);
int as_vocoder_hop(const as_vocoder* v);        /* samples per mel frame = the product of the rates (300) */
int as_vocoder_plan_create(const as_vocoder* v, as_plan** out);

typedef struct as_vocoder_io {
    const float* mel; int32_t ld_mel;           /* DEVICE [num_mels][ld_mel >= sum lens], packed frames */
    float* wav;                                 /* DEVICE [hop * sum lens] fp32 in [-1, 1], or NULL */
    int16_t* pcm;                               /* DEVICE [hop * sum lens] 16-bit PCM (as_conv_post_pcm_f32's rule), or NULL (at least one of the two) */
} as_vocoder_io;
/* lens_host int32 [B]: mel frames per utterance.  Workspace: caller-owned device memory, 256-byte aligned; 0 = invalid arguments. */
size_t as_vocoder_workspace_bytes(const as_vocoder* v, as_plan* p, int B, const int32_t* lens_host);
int as_vocoder_forward(const as_vocoder* v, as_plan* p, int B, const int32_t* lens_host, const as_vocoder_io* io,
                       void* ws, size_t ws_bytes, as_stream_t stream);
/* The same generator when the frame counts exist on the DEVICE only (predicted durations: as_forward_io.frame_cap): the launches are
 * sized by a capacity, one kernel derives every geometry table from `off` on the device (as_vocoder_cap_geometry, into the workspace), the
 * convolutions run under ConvGemmArgs.n_valid and the glue kernels under their valid counts.  Nothing is read back, nothing is uploaded,
 * the plan is not touched and NO call synchronises or allocates: every call -- the first included -- can be captured into a hipGraph and
 * replayed with other contents of off and mel, other lengths included.  Utterance b's samples are [sample_off[b], sample_off[b + 1]) =
 * hop * mult * off; wav / pcm in [hop * total, hop * cap) are written as 0 by the last kernel (no earlier request's samples remain).
 * More frames than cap, or an utterance longer than max_len: AS_STATUS_CAPACITY (as_device_status) -- the layout is cut at the
 * capacity, nothing is stored out of bounds, and that call's samples are not to be used.  Filler (mel columns past the total, the
 * workspace) may hold anything, NaNs included.
 * AS_EINVAL: mult < 1, cap < 1, max_len > cap, ld_mel < cap, hop * max_len > AS_META_MAX_W, both outputs NULL; AS_ENOSPC before anything
 * is launched; AS_EDEVICE while a status bit is set. */
typedef struct as_vocoder_cap {
    const int32_t* off;      /* DEVICE [B + 1], off[0] = 0: as_forward_io.frame_off, or prefix sums of mel lengths */
    int32_t mult;            /* mel frames per unit of off (2 for frame_off, 1 for mel lengths) */
    int32_t cap;             /* mel frames of room, all utterances: ld_mel >= cap, wav / pcm hold hop * cap samples */
    int32_t max_len;         /* mel frames the longest utterance may have (0 = cap): sizes the per-utterance grids */
    int32_t* sample_off;     /* optional DEVICE out [B + 1]: utterance b = samples [sample_off[b], sample_off[b + 1]) */
} as_vocoder_cap;
size_t as_vocoder_cap_workspace_bytes(const as_vocoder* v, as_plan* p, int B, int cap, int max_len);
int as_vocoder_forward_cap(const as_vocoder* v, as_plan* p, int B, const as_vocoder_cap* cap, const as_vocoder_io* io,
                           void* ws, size_t ws_bytes, as_stream_t stream);
/* Windowed vocoding (csrc/window.hip, csrc/vocoder_rt.hip; the rule: csrc/window_rule.h): the capacity call in
 * rounds of `core` mel frames per utterance -- the same inputs, the same output layout, the same samples within the module's bound -- with
 * a workspace that does not depend on the capacity and rounds that can be handed out one by one (streaming).
 * The generator is convolutions only, so a sample depends on the mel frames within a fixed radius: conv_pre 3 frames; per stage the 3-tap
 * phase conv 1 sample at the stage's input rate and the widest stack max_j (k_j / 2) (sum_n d_jn + n_dilations) samples at its output
 * rate; conv_post 3 samples.  halo = ceil(radius) frames: 12 for Vocoder/config.json (an upper bound).
 * The rule, per utterance of n mel frames (n as as_vocoder_cap_geometry lays it out: mult (off[b + 1] - off[b]) cut at cap and max_len;
 * a cut raises AS_STATUS_CAPACITY).  Round w: core frames [c0, c1) = [w core, min(n, (w + 1) core)), empty when w core >= n; source
 * frames [s0, s1) = [max(0, c0 - halo), min(n, c1 + halo)); skip = c0 - s0, count = c1 - c0.  The source is clamped to the utterance's
 * own ends: the window's zero padding is then the utterance's, first and last windows included.  woff [B + 1] = the prefix sums of
 * s1 - s0 over the batch (an ended utterance has an empty window): never more than core + 2 halo frames per utterance.
 * as_window_cfg: core >= 1; halo >= 0, or -1 = the generator's own (as_vocoder_* only); hop = samples per frame for the stitch called
 * alone (the as_vocoder_* calls use the generator's own and ignore it).
 * as_vocoder_halo_cfg    host only, no GPU: the halo in frames of a configuration; AS_EINVAL for one as_vocoder_create refuses.
 * as_window_host         the rule on HOST arrays: woff [B + 1], skip [B], count [B] of round `round`, *n_rounds = ceil(max_len / core)
 *                        (max_len 0 = cap), *over = 1 when the layout was cut (each pointer may be NULL).
 * as_window_gather_f32   one launch: mel [num_mels][ld_mel] -> the round's packed frames wmel [num_mels][ld_w], ld_w >= B (core + 2 halo);
 *                        woff DEVICE out [B + 1]; skip_count DEVICE out [2 B] = {skip, count} per utterance, or NULL.  Every workgroup
 *                        recomputes its utterance's offset from `off` (B <= 65535): no second launch.  Raises AS_STATUS_CAPACITY for a cut.
 * as_window_stitch_f32   one launch: the round's samples wwav [hop ld_w] (utterance b from hop woff[b]) -> each utterance's core samples
 *                        [hop skip, hop (skip + count)) at hop (o_b + round core) of wav fp32 and / or pcm (as_conv_post_pcm_f32's rule on
 *                        the fp32 value: a NaN stores 0 and raises AS_STATUS_F16_RANGE), each hop cap samples.  Round 0 also writes the
 *                        zeros of the filler [hop total, hop cap) and sample_off [B + 1] when given.  skip and count are derived from
 *                        `off` by the rule; a woff outside its buffer stores nothing and raises AS_STATUS_CAPACITY.
 * Both launches work on DEVICE offsets, read nothing back, upload and allocate nothing and can be captured.
 * as_vocoder_forward_windowed   rounds [round0, round0 + n_rounds) (n_rounds 0: all of them) of: gather, the launch sequence of
 *                        as_vocoder_forward_cap on woff with mult 1, cap B (core + 2 halo), max_len core + 2 halo into a window waveform in
 *                        the workspace, stitch.  cap / io as for as_vocoder_forward_cap; the outputs are those of that call.  Rounds are
 *                        independent but for round 0's duties: in pieces on one stream they give the bits of one call.  A round past every
 *                        utterance's end stores nothing.  Capturable like as_vocoder_forward_cap.
 * AS_EINVAL: core < 1, halo < -1, round0 < 0, n_rounds < 0, hop (core + 2 halo) > AS_META_MAX_W, both outputs NULL and
 * as_vocoder_forward_cap's own conditions but one: no utterance is laid out whole, so an utterance may be longer than AS_META_MAX_W
 * samples (hop cap < 2^31 is the limit); AS_ENOSPC before anything is launched; AS_EDEVICE while a status bit is set. */
typedef struct as_window_cfg { int32_t core, halo, hop; } as_window_cfg;
int as_vocoder_halo_cfg(const as_vocoder_cfg* cfg);
int as_vocoder_halo(const as_vocoder* v);
int as_window_host(const as_window_cfg* w, const int32_t* off_host, int B, int mult, int cap, int max_len, int round, int32_t* woff,
                   int32_t* skip, int32_t* count, int32_t* n_rounds, int32_t* over);
int as_window_gather_f32(const as_window_cfg* w, int round, const float* mel, int ld_mel, int num_mels, const int32_t* off, int B, int mult,
                         int cap, int max_len, float* wmel, int ld_w, int32_t* woff, int32_t* skip_count, as_stream_t stream);
int as_window_stitch_f32(const as_window_cfg* w, int round, const float* wwav, int ld_w, const int32_t* woff, const int32_t* off, int B,
                         int mult, int cap, int max_len, float* wav, int16_t* pcm, int32_t* sample_off, as_stream_t stream);
size_t as_vocoder_windowed_workspace_bytes(const as_vocoder* v, as_plan* p, int B, const as_window_cfg* w);
int as_vocoder_forward_windowed(const as_vocoder* v, as_plan* p, int B, const as_vocoder_cap* cap, const as_vocoder_io* io,
                                const as_window_cfg* w, int round0, int n_rounds, void* ws, size_t ws_bytes, as_stream_t stream);
/* Host helper (no GPU work): ConvTranspose1d weight wt [Cin][Cout][2u] (stride u, padding u/2 + u%2) -> the 3-tap conv
 * wc [u*Cout][Cin][3] whose output rows are (phase r, channel m), row r Cout + m:
 *     y[m][u q + r] = sum_c sum_d wc[r Cout + m][c][d] x[c][q + d - 1]
 * phase r reads tap kk = (r + p) % u + u j of wt at d = (r + p) / u - j + 1, j = 0, 1; the third entry of a row is zero. */
int as_vocoder_fold_upsample_host(const float* wt, int Cin, int Cout, int u, float* wc);

/* ---- sample-rate conversion (csrc/resample.hip; the rule: csrc/resample_rule.h) ---------------------------------
 * A polyphase windowed-sinc resampler over packed utterances: the reference wave at any rate in front of the mel front end, the
 * generator's 24 kHz samples at any rate behind it, without a host step.
 * The rule.  g = gcd(in_rate, out_rate), L = out_rate / g, M = in_rate / g, q = max(L, M).  Prototype filter at the rate in_rate * L, half
 * length H = 32 q: h[i] = fc sinc(fc i) kaiser(i) for i in [-H, H], fc = 0.915 / q, sinc(x) = sin(pi x) / (pi x), kaiser(i) =
 * I0(8.6 sqrt(1 - (i / H)^2)) / I0(8.6), scaled so that sum h = L; computed in double, rounded once to fp32.  An utterance of n_in samples
 * gives n_out = ceil(n_in L / M) samples,
 *     y[n] = sum_k h[n M - k L] x[k]     over 0 <= k < n_in with |n M - k L| <= H,
 * accumulated in fp32: an utterance sees zeros beyond its own ends, never a neighbour's samples, and an utterance in a batch equals the
 * same utterance alone bit for bit.
 * Limits (AS_EINVAL): a rate < 1, in_rate == out_rate, q > 640, M / L > 8 or L / M > 8.  Every pair among 8000, 11025, 12000, 16000,
 * 22050, 24000, 32000, 44100 and 48000 Hz is inside them but 11025 <-> 32000 (1280 / 441).
 * as_resample_design_host   no GPU work: L, M, H (each pointer may be NULL) and, taps != NULL, the prototype h[-H .. H] as fp32
 *                           taps[0 .. 2 H] (AS_EINVAL if n_taps < 2 H + 1); taps == NULL: sizes only.
 * as_resampler_create       designs the filter and uploads its phase table to the current HIP device (allocates, synchronises).  The
 *                           handle is immutable: any number of calls, streams and threads may share it.
 * as_resample_f32           in_off DEVICE int32 [B + 1], in_off[0] = 0: utterance b is x[in_off[b] .. in_off[b + 1]) (an
 *                           as_vocoder_cap.sample_off, or prefix sums of known lengths); x DEVICE [in_cap].  Outputs, each out_cap
 *                           samples, packed from 0: y fp32 and / or pcm 16-bit (as_conv_post_pcm_f32's rule applied to the fp32 value in
 *                           the same pass: a NaN stores 0 and raises AS_STATUS_F16_RANGE), at least one of the two; out_off (optional,
 *                           DEVICE [B + 1]) = the prefix sums of ceil(len_b L / M).  The lengths exist on the device only: ONE launch, sized
 *                           by out_cap, derives the layout and resamples.  Nothing is read back, uploaded or allocated and no call
 *                           synchronises: every call, the first included, can be captured into a hipGraph and replayed with other
 *                           offsets and samples.  y / pcm in [out_off[B], out_cap) are written as 0.  More output than out_cap, or
 *                           in_off[B] > in_cap: AS_STATUS_CAPACITY -- the layout is cut at the capacities, nothing is read or stored out
 *                           of bounds, and that call's samples are not to be used.
 *                           AS_EINVAL before anything is launched: r, in_off or x NULL, both outputs NULL, B < 1, in_cap < 1, out_cap < 1,
 *                           in_cap * L >= 2^31 or out_cap * M >= 2^31; AS_EDEVICE while a status bit is set. */
typedef struct as_resampler as_resampler;
int as_resample_design_host(int in_rate, int out_rate, int32_t* L, int32_t* M, int32_t* H, float* taps, int n_taps);
int as_resampler_create(int in_rate, int out_rate, as_resampler** out);
int as_resampler_destroy(as_resampler* r);
int as_resampler_info(const as_resampler* r, int32_t* L, int32_t* M, int32_t* H);
int as_resample_f32(const as_resampler* r, int B, const int32_t* in_off, int in_cap, const float* x, int out_cap, float* y, int16_t* pcm,
                    int32_t* out_off, as_stream_t stream);

/* ---- paragraphs: a batch's utterances as streams (csrc/join.hip; the rule: csrc/join_rule.h) ---------------------
 * A page of text is synthesised as a batch of its sentences; the joiner turns the packed samples of that batch into G streams on the
 * device: every utterance trimmed of the silence at its ends, levelled against the others, faded at the cuts, with pauses between.
 * The rule, per utterance x[0 .. n), F = cfg->frame.  Blocks: K = ceil(n / F), block k has cnt_k = min(F, n - k F) samples, ss_k = its fp32
 * sum of squares (in the one order join_rule.h fixes), pk_k = max |x|, ms_k = ss_k / cnt_k, top = max ms_k.  Trim (trim_ratio > 0, a power
 * ratio 10^(-dB / 10)): block k is active when ms_k > 0 and ms_k >= fp32(trim_ratio * top); k0, k1 = first and last active block; kept
 * [s0, s1) = [max(0, k0 F - keep), min(n, (k1 + 1) F + keep)), empty when no block is active; trim off: all blocks active, [0, n).  Level
 * (target_rms > 0): A = sum ss_k and C = sum cnt_k over the active blocks, rms = sqrtf(A / C), peak = max pk_k over all blocks,
 * g = min(target_rms / rms, peak_ceiling / peak, max_gain); g = 1 when A == 0 or the level is off.  Edges: m = s1 - s0, f = min(fade, m / 2),
 * w(i) = (i + 0.5) / f for i < f, (m - 1 - i + 0.5) / f for i >= m - f, else 1; y_i = (x[s0 + i] g) w(i).  Layout: group_off [G + 1] cuts the
 * B utterances into G streams (a group may be empty); a stream is `lead` zeros, its non-empty pieces in order, `tail` zeros, with
 * max(gap[b], 0) zeros (cfg->gap without an array) in front of every piece that is not the first non-empty one of its stream; an empty
 * piece adds nothing and its gap is dropped.  An utterance in a batch gives the bits of the same utterance joined alone; with the trim
 * and the level off and fade = gap = lead = tail = 0 and one group the output is the packed input bit for bit.
 * as_join_io: in_off DEVICE int32 [B + 1] (in_off[0] = 0; an as_vocoder_cap.sample_off, an as_resample_f32 out_off, or prefix sums of
 * known lengths), x DEVICE [in_cap]; group_off DEVICE [G + 1] or NULL (one stream; inner cuts are read clamped to [0, B]), gap DEVICE [B] or
 * NULL; outputs, each out_cap samples: y fp32 and / or pcm (as_conv_post_pcm_f32's rule on the fp32 value), samples in [out_off[G], out_cap)
 * are 0; optional out_off [G + 1], piece [B] (where utterance b landed and which of its own samples were kept: subtitles, lip-sync; an empty
 * piece has out_start == out_end) and gain [B].
 * as_join_f32           three launches (measure, reduce, write), sized by in_cap and out_cap: nothing is read back, uploaded or allocated
 *                       and no call synchronises -- every call, the first included, can be captured into a hipGraph and replayed with other
 *                       offsets, samples and gaps.  The streams need more than out_cap, or in_off[B] > in_cap: AS_STATUS_CAPACITY (the layout
 *                       is cut at the capacities, nothing is read or stored out of bounds); a sample that is not finite:
 *                       AS_STATUS_F16_RANGE; either way that call's output is void.
 * as_join_measure_f32   the first two launches only: piece[b].src_start / src_end = the kept range (out_start = out_end = 0), gain if
 *                       given; y, pcm, out_cap, group_off and gap are not read.  The device trim of a reference wave.
 * as_join_host          the same rule on HOST arrays (every pointer of io is a host pointer; no GPU, no workspace): io->y or io->pcm given:
 *                       the join; neither: the measurement, into io->piece.  AS_ENOSPC: the streams need more than out_cap (the output is
 *                       cut there); AS_EDEVICE: a sample is not finite; AS_EINVAL also for offsets that do not ascend from 0 to <= in_cap.
 * AS_EINVAL before anything is launched: cfg, io, ws, in_off or x NULL, B < 1, G < 1, both outputs NULL (measure: piece NULL), frame outside
 * [16, 4096], negative keep / fade / lead / tail, a negative or non-finite float, in_cap or out_cap below 1 or above 2^30.  AS_ENOSPC: ws_bytes below
 * as_join_workspace_bytes(B, in_cap, cfg) (0 for arguments it refuses).  AS_EDEVICE while a status bit is set. */
typedef struct as_join_cfg {
    int32_t frame;                 /* samples per measuring block */
    float trim_ratio;              /* 0: no trim */
    int32_t keep, fade, gap, lead, tail;   /* samples */
    float target_rms, peak_ceiling, max_gain;   /* target_rms 0: no levelling */
} as_join_cfg;
typedef struct as_join_piece {
    int32_t out_start, out_end, src_start, src_end;
} as_join_piece;
typedef struct as_join_io {
    const int32_t* in_off; int32_t in_cap;
    const float* x;
    int32_t G; const int32_t* group_off;
    const int32_t* gap;
    int32_t out_cap;
    float* y; int16_t* pcm;
    int32_t* out_off;
    as_join_piece* piece;
    float* gain;
} as_join_io;
size_t as_join_workspace_bytes(int B, int in_cap, const as_join_cfg* cfg);
int as_join_f32(const as_join_cfg* cfg, int B, const as_join_io* io, void* ws, size_t ws_bytes, as_stream_t stream);
int as_join_measure_f32(const as_join_cfg* cfg, int B, const as_join_io* io, void* ws, size_t ws_bytes, as_stream_t stream);
int as_join_host(const as_join_cfg* cfg, int B, const as_join_io* io);

/* ---- mastering: programme loudness and a true-peak limiter (csrc/master.hip; the rule: csrc/master_rule.h) --------
 * The last stage of the sample back end: G packed streams are brought to a programme loudness (ITU-R BS.1770: K-weighted, gated) and held
 * under a true-peak ceiling by a look-ahead limiter.  No length changes: offsets, pieces and speech marks stay valid as they are.
 * The rule, per stream x[0 .. n) at cfg->rate Hz (zeros beyond its ends, never a neighbour's samples).  K-weighting: the shelf and the
 * high pass of BS.1770 designed in double for the rate by the bilinear transform (at 48 kHz the standard's table), rounded once to fp32,
 * each in transposed direct form II.  The recurrence is cut into chunks of P = 512 samples from the stream's OWN first sample: every chunk
 * filtered from the zero state gives its final state f_j; S_0 = 0, S_{j+1} = T S_j + f_j with T the P-step transition matrix (double,
 * rounded once); every chunk is filtered again from S_j.  hop = rate / 10; e_i = the sum of squares of the filter's output over hop i;
 * block i = hops i .. i + 3, z_i = (e_i + .. + e_{i+3}) / (4 hop), complete blocks only; a stream shorter than one block has ONE block,
 * z = sum / n.  Gates: z_i > abs_gate (10^((-70 + 0.691) / 10)), then z_i > 0.1 x the mean of the absolutely gated z; power = the mean of
 * the z that pass both (0: none passes the absolute gate); the loudness is -0.691 + 10 log10(power) LUFS (computed by the caller: the rule
 * has no logarithm).  Gain: g = min(sqrt(target_power / power), max_gain), 1 when power == 0 or target_power == 0 (loudness off;
 * target_power = 10^((LUFS + 0.691) / 10)).  True peak: the resampler's own prototype for L = 4, M = 1 (64 taps per phase),
 * p[n] = max(|g x[n]|, |g d_j[n]|, j = 0..3), d_j = phase j at sample n.  Limiter (ceiling > 0; A = lookahead samples, 1..512):
 * r[n] = min(1, ceiling / p[n]), 1 outside the stream; c[k] = min r[k .. k + A]; s[n] = (c[n - A] + .. + c[n]) / (A + 1);
 * y[n] = (g x[n]) s[n].  Hence |y[n]| <= ceiling (1 + 2^-14); y = g x bit for bit where nothing within +-A samples is over the ceiling; no
 * delay; the gain is not raised again behind the limiter, so the loudness of a limited stream may sit a little under the target, and the
 * TRUE peak of y may pass the ceiling by a few hundredths of a dB.  Every order of operations is fixed by master_rule.h: a
 * stream in a batch gives the bits of the same stream alone, and the device gives the bits of as_master_host.  Loudness and ceiling off:
 * the output is the input bit for bit.  An empty stream writes nothing; its report is power 0, gain 1, peak 0, floor 1.
 * as_master_io: in_off DEVICE int32 [G + 1] (in_off[0] = 0; an as_join_f32 or as_resample_f32 out_off, an as_vocoder_cap.sample_off, or
 * prefix sums), x DEVICE [in_cap]; outputs, each in_cap samples at the offsets of the input: y fp32 and / or pcm (as_conv_post_pcm_f32's
 * rule on the fp32 value: a NaN stores 0 and raises AS_STATUS_F16_RANGE), samples in [in_off[G], in_cap) are 0; report DEVICE [G]
 * (optional for as_master_f32): power, gain, peak = max p[n], floor = min s[n], blocks, gated = the blocks that passed both gates.
 * as_master_design_host   no GPU: the ten coefficients in double (b0 b1 b2 a1 a2 of the shelf, then of the high pass), T [4][4] as the
 *                         kernels use it (the P-th power, in double, of the one-step state matrix of the fp32 coefficients, rounded
 *                         once), P and hop; each pointer may be NULL.
 * as_master_create        validates the cfg and designs the filters and the oversampler's phase table on the host.  The handle is
 *                         immutable and holds no device memory (the tables travel as kernel arguments): any number of calls, streams,
 *                         threads and devices may share it, and it is created without a GPU.
 * as_master_f32           at most five launches sized by in_cap (filter, carry, refilter with hop energies, gates with gain and report,
 *                         limiter with the stores); loudness off: the report's initialisation and the limiter.  Nothing is read back,
 *                         uploaded or allocated and no call synchronises: every call, the first included, can be captured into a hipGraph
 *                         and replayed with other offsets and samples.  in_off[G] > in_cap: AS_STATUS_CAPACITY (the layout is cut there,
 *                         nothing is read or stored out of bounds).  With loudness off the report's power, blocks and gated are 0.
 *                         y == x is refused (AS_EINVAL): a tile's halo lies in its neighbours' outputs, and a second launch is not spent
 *                         on it.
 * as_master_measure_f32   the meter: the report only -- the loudness whatever target_power says, gain = what WOULD be applied, peak = the
 *                         true peak of g x, floor 1; y and pcm are not read.
 * as_master_host          the same rule on HOST arrays (every pointer of io is a host pointer; no GPU, no workspace): io->y or io->pcm
 *                         given: the stage (y == x is allowed here); neither: the meter.  AS_EDEVICE: a NaN went to pcm; AS_EINVAL also for
 *                         offsets that do not ascend from 0 to <= in_cap.
 * AS_EINVAL before anything is launched: m, io, ws, in_off or x NULL, both outputs NULL (measure: report NULL), G outside [1, 65535], in_cap
 * outside [1, 2^30]; from as_master_create and as_master_host: rate outside [8000, 192000], lookahead outside [1, 512] with ceiling > 0, a
 * negative or non-finite float.  AS_ENOSPC: ws_bytes below as_master_workspace_bytes(G, in_cap, cfg) (0 for arguments it refuses).
 * AS_EDEVICE while a status bit is set. */
typedef struct as_master_cfg {
    int32_t rate;                  /* samples per second of the streams */
    float target_power, abs_gate, max_gain;   /* linear; target_power 0: loudness off */
    float ceiling;                 /* linear; 0: limiter off */
    int32_t lookahead;             /* samples */
} as_master_cfg;
typedef struct as_master_report {
    float power, gain, peak, floor;
    int32_t blocks, gated;
} as_master_report;
typedef struct as_master_io {
    const int32_t* in_off; int32_t in_cap;
    const float* x;
    float* y; int16_t* pcm;
    as_master_report* report;
} as_master_io;
typedef struct as_master as_master;
int as_master_design_host(int rate, double* biquads10, float* carry16, int32_t* P, int32_t* hop);
int as_master_create(const as_master_cfg* cfg, as_master** out);
int as_master_destroy(as_master* m);
size_t as_master_workspace_bytes(int G, int in_cap, const as_master_cfg* cfg);
int as_master_f32(const as_master* m, int G, const as_master_io* io, void* ws, size_t ws_bytes, as_stream_t stream);
int as_master_measure_f32(const as_master* m, int G, const as_master_io* io, void* ws, size_t ws_bytes, as_stream_t stream);
int as_master_host(const as_master_cfg* cfg, int G, const as_master_io* io);

/* ---- speech marks (csrc/marks.hip; the rule: csrc/marks_rule.h) ---------------------------------------------------
 * When every token is spoken in the samples the caller receives, and the twelve tracks the predictors hand the decoder (F0, N, EMA 0..9)
 * retimed onto an animation clock of fps_num / fps_den frames per second of those samples -- behind the duration rounding, the hop, the
 * resampler's ceil(n L / M) and the joiner's trim and placement, all of which exist on the device only.
 * as_marks_cfg: hop = samples per full-rate column at 24 kHz (as_vocoder_hop), L / M = the resampler's ratio (as_resampler_info; 1 / 1
 * without one), rate = samples per second of the final stream, fps_num / fps_den = the animation clock (30000 / 1001 is exact).
 * The rule.  fcap = min(ld_pred / 2, 2^24) with tracks, else 2^24.  Utterance b: f0 = clamp(frame_off[b], 0, fcap), f1 = clamp(frame_off[b + 1],
 * f0, fcap), its columns are [col0, col0 + W_b) with col0 = 2 f0, W_b = 2 (f1 - f0); r(p) = ceil(p L / M); n_b = min(r(hop W_b), 2^30).
 * Placement with `piece` (an as_join_f32 result, with the G, group_off and out_off of that call): utterance b lies in stream grp_b = the
 * number of inner cuts group_off[1 .. G) at or below b (no group_off: G = 1), stream g = [s_g, e_g) = out_off[g], out_off[g + 1] clamped to
 * [0, 2^30] and e_g >= s_g; os = clamp(out_start, s_g, e_g), oe = clamp(out_end, os, e_g), ss = clamp(src_start, 0, n_b), se = clamp(src_end, ss,
 * n_b), m = min(oe - os, se - ss): kept samples [ss, ss + m) at [os, os + m); the pieces of a stream ascend.  Without `piece`: G = B, every
 * utterance is a stream of its own at the prefix sums of n_b (= as_vocoder_cap.sample_off, or as_resample_f32's out_off), ss = 0, m = n_b.
 * Token marks: the tokens of utterance b are [t0, t1) = tok_off[b], tok_off[b + 1] clamped to [0, n_tokens] and ascending, d_k = max(dur_i[k],
 * 0), e_k = min(sum of d over [t0, k), W_b / 2); mark(e) = os + clamp(r(2 hop e) - ss, 0, m); marks[k] = {mark(e_k), mark(min(e_k + d_k,
 * W_b / 2))}, absolute sample positions in the output buffer, monotone inside an utterance; a token the trim removed entirely has start ==
 * end.  Packed tokens outside every [t0, t1) are not written.
 * Tracks: stream g has n_g = floor((e_g - s_g - 1) num / (rate den)) + 1 frames (0 when empty), anim_off = their prefix sums; frame m stands at
 * q = s_g + m den rate / num, exactly: Q = m den rate + s_g num.  b* = the last piece of the stream with os num <= Q; Q < oe(b*) num: inside,
 * active = 1: A = (Q - (os - ss) num) M, D = num L hop, x = (2 A - D) / (2 D) (column j has its midpoint at j + 1/2), j = floor(x); j < 0:
 * column 0; j >= W_b - 1: column W_b - 1; else w = fp32(double(2 A - D - 2 D j) / double(2 D)) clamped to [0, 1] and the value of track c is
 * fmaf(w, v[j + 1] - v[j], v[j]), v[j] = row c at column col0 + j.  Else active = 0; a / c = the nearest non-empty piece of the stream at or
 * before / behind b*; E_a = a's value at A = se num M, S_c = c's value at A = ss num M; both: fmaf(wg, S_c - E_a, E_a) with
 * wg = fp32(double(Q - oe_a num) / double((os_c - oe_a) num)) clamped to [0, 1]; only c (the lead): S_c; only a (the tail): E_a; neither
 * (a stream without a non-empty piece): 0.  scale / offset (both or neither, [12]): every value but those zeros becomes
 * fmaf(scale[c], value, offset[c]).  tracks and active in [anim_off[G], anim_cap) are 0.
 * as_marks_io: DEVICE pointers.  Inputs: tok_off [B + 1] and dur_i [n_tokens] (read for marks only), frame_off [B + 1], F0 / N / EMA with
 * ld_pred (as_forward_io's, read for tracks only); optional piece [B] with G, group_off [G + 1] or NULL, out_off [G + 1] (required with
 * piece); optional scale, offset.  Outputs, each optional, at least one: marks [n_tokens][2] (8-byte aligned), tracks [12][ld_tracks >=
 * anim_cap], active [anim_cap], anim_off [G + 1] ([B + 1] without piece).
 * as_marks_f32          at most three launches (layout, token marks, tracks), sized by B, n_tokens and anim_cap: nothing is read back,
 *                       uploaded or allocated and no call synchronises -- every call, the first included, can be captured into a hipGraph and
 *                       replayed with other durations, pieces and tracks.  The frames need more than anim_cap, or an offset, a piece or a
 *                       stream had to be clamped: AS_STATUS_CAPACITY -- the layout is cut at the capacities, nothing is read or stored out of
 *                       bounds, and that call's output is void.
 * as_marks_host         the same rule on HOST arrays (every pointer of io is a host pointer; no GPU, no workspace); AS_ENOSPC where the
 *                       device raises AS_STATUS_CAPACITY.
 * AS_EINVAL before anything is launched: cfg, io, ws or frame_off NULL; no output; marks without tok_off / dur_i; piece without out_off, or
 * without group_off and G != 1; tracks without F0 / N / EMA, with ld_pred < 2 or ld_tracks < anim_cap; tracks or active with anim_cap < 1;
 * one of scale and offset; outside the rule's limits: hop in [1, 2^16], L, M in [1, 2^12], rate in [1, 2^20], fps_num, fps_den in [1, 2^16],
 * B in [1, 2^20], n_tokens, anim_cap in [0, 2^30], G in [1, 4096] with piece.  AS_ENOSPC: ws_bytes below as_marks_workspace_bytes(B,
 * n_tokens, cfg) (0 for arguments it refuses).  AS_EDEVICE while a status bit is set. */
typedef struct as_marks_cfg {
    int32_t hop, L, M, rate, fps_num, fps_den;
} as_marks_cfg;
typedef struct as_marks_io {
    const int32_t* tok_off; const int32_t* dur_i;
    const int32_t* frame_off;
    const float* F0; const float* N; const float* EMA; int32_t ld_pred;
    const as_join_piece* piece; int32_t G; const int32_t* group_off; const int32_t* out_off;
    const float* scale; const float* offset;
    int32_t* marks;
    float* tracks; int32_t ld_tracks; int32_t anim_cap;
    uint8_t* active;
    int32_t* anim_off;
} as_marks_io;
size_t as_marks_workspace_bytes(int B, int n_tokens, const as_marks_cfg* cfg);
int as_marks_f32(const as_marks_cfg* cfg, int B, int n_tokens, const as_marks_io* io, void* ws, size_t ws_bytes, as_stream_t stream);
int as_marks_host(const as_marks_cfg* cfg, int B, int n_tokens, const as_marks_io* io);

/* ---- cue tracks: pieces at absolute times, mixed over a ducked bed (csrc/cues.hip; the rule: csrc/cue_rule.h) ------
 * The joiner lays pieces out back to back; this stage puts every piece AT A TIME on one of G tracks (a speaker each, say), and can mix the
 * tracks over a music-and-effects bed that is ducked under the speech.  Its stems are packed streams with an out_off (as_master_f32 takes
 * them as they are), its piece table is an as_join_piece table (as_marks_f32 takes it with the same G, group_off and out_off).
 * The rule.  Piece b = x[in_off[b] .. in_off[b + 1]) (read clamped to [0, in_cap]), n_b samples; group_off [G + 1] cuts the B pieces into G
 * tracks as the joiner's does (inner cuts clamped to [0, B]; NULL: everything on track 0).  Layout, per track in batch order, E = 0 the
 * running end, any = "a non-empty piece has been placed": s_b = max(start[b], 0); p_b = max(s_b, E + (any ? min_gap : 0)); m_b = n_b, cut to
 * max(limit[b] - p_b, 0) with a limit (limit given and limit[b] > 0) and to max(track_len - p_b, 0) with track_len > 0; cut_b = n_b - m_b,
 * late_b = p_b - s_b.  m_b > 0: the piece lies at [p_b, p_b + m_b), E = p_b + m_b, any is set; else it lies nowhere, E stays, and piece[b] has
 * out_start = out_end = E (a track's pieces ascend).  A track is track_len samples long when track_len > 0, else E + tail, and 0 without a
 * placed piece; out_off = the prefix sums.  Samples: y[out_off[g] + p_b + i] = (x_b[i] gain[b]) w_b(i) for i < m_b (gain NULL: 1); w_b = 1 but
 * for a piece with cut_b > 0, whose last f = min(fade, m_b) samples take w = ((m_b - 1 - i) + 0.5) / f.  Everything else of a track is 0, and
 * so is [out_off[G], out_cap).  piece[b] = {out_off[g] + p_b, out_off[g] + p_b + m_b, src0, src0 + m_b} with src0 = piece_in[b].src_start
 * (piece_in: the as_join_piece table of a joiner run with one group per utterance, whose output x is; NULL: 0); report[b] = {p_b, late_b,
 * cut_b, g}.  Mix (mix or mix_pcm given; G <= 64): T = the longest track; speech(t) = the tracks' samples added in ascending track order
 * from 0.f (0 behind a track's end); cover c(t) = the maximum over placed pieces of r_b(t), e_b = p_b + m_b: 1 on [p_b, e_b + hold),
 * (t - (p_b - attack) + 1) / (attack + 1) on [p_b - attack, p_b), (e_b + hold + release - t) / (release + 1) on [e_b + hold, e_b + hold + release),
 * else 0; k = 1 - depth; duck(t) = fmaf(-k, c(t), 1); mix(t) = bed(t) (bed_gain duck(t)) + speech(t) with bed(t) = bed[t] for t < bed_n, else 0
 * (no bed: 0); mix_off = {0, T}; [T, mix_cap) is 0.  depth is the bed's linear gain at full duck: 1 = no ducking.  Every fp32 operation has
 * one rounding in the order cue_rule.h fixes: a track alone gives the bits of the same track in a batch, the device those of as_cue_host.
 * as_cue_io: DEVICE pointers.  in_off [B + 1], x [in_cap], start [B]; optional group_off [G + 1], limit [B], gain [B], piece_in [B], bed
 * [bed_n].  Outputs, each optional, at least one of y, pcm, mix, mix_pcm: y fp32 / pcm (as_conv_post_pcm_f32's rule on the fp32 value: a NaN
 * stores 0 and raises AS_STATUS_F16_RANGE) [out_cap], out_off [G + 1], piece [B], report [B]; mix / mix_pcm [mix_cap], mix_off [2].
 * as_cue_f32            at most three launches (layout, write, mix), sized by B, out_cap and mix_cap: nothing is read back, uploaded or
 *                       allocated and no call synchronises -- every call, the first included, can be captured into a hipGraph and replayed
 *                       with other offsets, starts and samples.  The tracks need more than out_cap, T > mix_cap, in_off[B] > in_cap, or a
 *                       position beyond 2^30: AS_STATUS_CAPACITY (the layout is cut there, nothing is read or stored out of bounds; that
 *                       call's output is void).  y == x and mix == bed are refused.  With a mix and no y the stems go to the workspace.
 * as_cue_host           the same rule on HOST arrays (every pointer of io is a host pointer; no GPU, no workspace).  AS_ENOSPC where the
 *                       device raises AS_STATUS_CAPACITY; AS_EDEVICE: a NaN went to pcm; AS_EINVAL also for offsets that do not ascend from
 *                       0 to <= in_cap.
 * AS_EINVAL before anything is launched: cfg, io, ws, in_off, x or start NULL; no sample output; B outside [1, 65536]; G outside [1, 4096],
 * or above 64 with a mix; in_cap, out_cap (mix_cap with a mix) outside [1, 2^30]; min_gap, fade, tail, attack, hold, release outside
 * [0, 2^20]; track_len outside [0, 2^30]; depth outside [0, 1]; bed_gain negative or not finite; bed_n < 0 with a bed.  AS_ENOSPC: ws_bytes
 * below as_cue_workspace_bytes(B, G, in_cap, out_cap, mix_cap, cfg) (mix_cap 0: no mix; 0 for arguments it refuses).  AS_EDEVICE while a
 * status bit is set. */
typedef struct as_cue_cfg {
    int32_t min_gap, fade, tail;   /* samples: between two pieces of a track, the fade-out of a cut piece, behind a track's last piece */
    int32_t track_len;             /* samples; 0: as long as needed */
    int32_t attack, hold, release; /* samples: the duck's ramp down, its hold behind a piece and its ramp up */
    float depth, bed_gain;         /* linear: the bed's gain at full duck (1: no ducking), the bed's gain */
} as_cue_cfg;
typedef struct as_cue_report {
    int32_t pos, late, cut, track; /* p_b, late_b, cut_b, g */
} as_cue_report;
typedef struct as_cue_io {
    const int32_t* in_off; int32_t in_cap;
    const float* x;
    int32_t G; const int32_t* group_off;
    const int32_t* start; const int32_t* limit; const float* gain; const as_join_piece* piece_in;
    int32_t out_cap;
    float* y; int16_t* pcm;
    int32_t* out_off;
    as_join_piece* piece;
    as_cue_report* report;
    const float* bed; int32_t bed_n;
    int32_t mix_cap;
    float* mix; int16_t* mix_pcm;
    int32_t* mix_off;
} as_cue_io;
size_t as_cue_workspace_bytes(int B, int G, int in_cap, int out_cap, int mix_cap, const as_cue_cfg* cfg);
int as_cue_f32(const as_cue_cfg* cfg, int B, const as_cue_io* io, void* ws, size_t ws_bytes, as_stream_t stream);
int as_cue_host(const as_cue_cfg* cfg, int B, const as_cue_io* io);

/* ---- rooms: convolution reverb on packed streams and as a send on a mix (csrc/room.hip; the rule: csrc/room_rule.h) ----
 * A bank of K impulse responses -- designed rooms, measured rooms, a telephone's or a radio's FIR -- laid over G packed streams, each stream
 * with its own response, send, dry gain and predelay; or, over the stems and the mix of as_cue_f32, added to the mix as a send.
 * The rule.  Stream g = x[in_off[g] .. in_off[g + 1]) (read clamped to [0, in_cap]), n_g samples; response k = h[ir_off[k] .. ir_off[k + 1])
 * (clamped to [0, ir_cap]), L_k taps, cut at 2^17 (AS_STATUS_CAPACITY); L_k = 0 is a wet signal of 0.  Per stream, DEVICE arrays [G] read when
 * the call RUNS: room[g] an index into the bank (< 0: dry only; >= K: dry only and AS_STATUS_BAD_LAYOUT), send[g] the linear wet gain, dry[g]
 * (NULL: 1), delay[g] the predelay in samples (NULL: 0; clamped to [0, 2^20]).  Wet signal, for every t >= 0: acc = 0.f; for k = 0 .. L - 1
 * ASCENDING, j = t - delay - k, 0 <= j < n_g: acc = fmaf(h[k], x_g[j], acc); c_g(t) = acc -- one rounding per tap, one order, never a
 * neighbour's sample: a stream alone gives the bits it has in a batch, the device those of as_room_host.  A non-finite tap is the caller's
 * error (the output is then not finite; nothing is read or stored out of bounds).
 * Streams mode (mix_in NULL): output stream g has m_g = n_g + cfg->tail samples (0 for an empty stream), out_off = the prefix sums;
 * y_g[t] = fmaf(send_g, c_g(t), dry_g xz_g(t)), xz = x inside the stream and 0 in the tail; without a valid room y_g[t] = dry_g xz_g(t);
 * [out_off[G], out_cap) is 0.  tail = 0, every room negative, dry NULL: the output is the input bit for bit.  piece (optional): without
 * piece_in piece[g] = {out_off[g], out_off[g] + n_g, 0, n_g}; with piece_in [B] and group_off [G + 1] (a joiner's or the cue stage's table
 * of the streams) every piece of stream g has out_start / out_end moved by out_off[g] - (stream g's first input sample), src_* as they
 * were -- what as_marks_f32 needs to stay valid under a tail.  y == x is refused: a tile's history lies in its neighbour's output.
 * Return mode (mix_in given; the streams are stems on ONE timeline from 0, as as_cue_f32 writes them; G <= 64): T = clamp(mix_off[1], 0,
 * mix_cap), read on the device; for t < T: a = mix_in[t], for g ascending with a valid room a = fmaf(send_g, c_g(t), a), mix[t] = a -- a
 * stem rings on behind its own end up to T; [T, mix_cap) is 0.  dry, tail, out_off and piece are not used; y or pcm are refused;
 * mix == mix_in is allowed.
 * as_room_io: DEVICE pointers.  Outputs fp32 and / or 16-bit PCM (as_conv_post_pcm_f32's rule on the fp32 value: a NaN stores 0 and raises
 * AS_STATUS_F16_RANGE).
 * as_room_f32           at most two launches, sized by out_cap or by G and mix_cap -- streams mode: the samples, whose job search is the
 *                       layout, and the pieces with a piece_in; return mode: the stems' wet signals into the workspace (G rows of mix_cap
 *                       samples: every stem's tiles run side by side), then their sum onto the mix in ascending order.  Nothing is read
 *                       back, uploaded or allocated and no call synchronises -- every call, the first included,
 *                       can be captured into a hipGraph and replayed with other offsets, samples, taps, rooms and sends.  The streams need
 *                       more than out_cap, in_off[G] > in_cap or mix_off[1] > mix_cap: AS_STATUS_CAPACITY (the layout is cut there, nothing
 *                       is read or stored out of bounds; that call's output is void).
 * as_room_host          the same rule on HOST arrays (every pointer of io is a host pointer; no GPU, no workspace).  AS_ENOSPC where the
 *                       device raises AS_STATUS_CAPACITY; AS_EDEVICE: a NaN went to pcm, or a room index was >= K.
 * as_room_design_host   host only: a room from four numbers, in double, rounded once.  Ls = rt60_ms rate / 1000, L = clamp(ceil(Ls), 1, 2^17);
 *                       u(k) = int32(lowbias32(seed 0x9E3779B9 + k)) / 2^31; v[k] = u(k) exp(-ln(1000) k / Ls); w[k] = (1 - damping) v[k] +
 *                       damping w[k - 1]; h = w / sqrt(sum w^2) -- unit energy, so that a send in dB means something.  *n_taps = L; h NULL
 *                       asks for the length only; AS_ENOSPC: h_cap < L; AS_EINVAL: rate outside [1, 768000], rt60_ms outside [1, 3600000],
 *                       damping outside [0, 0.95].
 * as_room_geometry      the sample kernel's tile (outputs of one stream per workgroup) and chunk (taps staged at a time).
 * AS_EINVAL before anything is launched: cfg, io, ws, in_off, x, ir_off, h, room or send NULL; no sample output; both modes' outputs; mix
 * outputs without mix_in or the reverse; y == x; G outside [1, 65535], or above 64 in return mode; K outside [1, 4096]; in_cap, ir_cap,
 * out_cap (streams mode), mix_cap (return mode) outside [1, 2^30]; tail outside [0, 2^20]; piece_in without group_off or with B outside
 * [1, 65536]; mix_in without mix_off.  AS_ENOSPC: ws_bytes below as_room_workspace_bytes(G, in_cap, out_cap, mix_cap, cfg) (the capacity of
 * the mode that is not used: 0; returns 0 for arguments it refuses).  AS_EDEVICE while a status bit is set. */
typedef struct as_room_cfg {
    int32_t tail, reserved;        /* samples behind every stream for the ring-out (streams mode); 0 */
} as_room_cfg;
typedef struct as_room_io {
    const int32_t* in_off; int32_t in_cap;
    const float* x;
    int32_t K; const int32_t* ir_off; int32_t ir_cap;
    const float* h;
    const int32_t* room; const float* send; const float* dry; const int32_t* delay;
    int32_t out_cap;
    float* y; int16_t* pcm;
    int32_t* out_off;
    int32_t B; const int32_t* group_off; const as_join_piece* piece_in;
    as_join_piece* piece;
    const float* mix_in; const int32_t* mix_off; int32_t mix_cap;
    float* mix; int16_t* mix_pcm;
} as_room_io;
typedef struct as_room_design {
    int32_t rate, rt60_ms;         /* samples per second; the time the response takes to fall by 60 dB */
    float damping;                 /* the one-pole low-pass on the noise: 0 white .. 0.95 dark */
    uint32_t seed;
} as_room_design;
size_t as_room_workspace_bytes(int G, int in_cap, int out_cap, int mix_cap, const as_room_cfg* cfg);
int as_room_f32(const as_room_cfg* cfg, int G, const as_room_io* io, void* ws, size_t ws_bytes, as_stream_t stream);
int as_room_host(const as_room_cfg* cfg, int G, const as_room_io* io);
int as_room_design_host(const as_room_design* d, float* h, int32_t h_cap, int32_t* n_taps);
int as_room_geometry(int32_t* tile, int32_t* chunk);

/* ---- prosody transfer (csrc/dtw.hip, csrc/dtw_rule.h) -------------------------------------------------------------
 * Speak a sentence the way a recording of it was spoken: synthesise it once (pass A), warp pass A's mel onto the recording's log-mel
 * (dynamic time warping, frame by frame), turn the warp into one prosody row per token (as_plan_set_token_prosody's rows: a duration scale
 * and twelve track offsets) and synthesise again with those rows (pass B).  Nothing here synchronises, allocates or reads back; every
 * length is DEVICE data, so the whole chain can be captured into a hipGraph and replayed with other contents.
 * The rule (csrc/dtw_rule.h states it in full).  Cost of synthesised frame i and recording frame j over C <= AS_DTW_MAX_C bins: acc = 0,
 * for k in order d = a_k(i) - b_k(j), acc = fmaf(d, d, acc); center = 1 takes each side's per-bin mean over its own frames (fp32 sum in
 * ascending frame order / fp32(count)) off first: d = (a_k(i) - ma_k) - (b_k(j) - mb_k) -- what makes another speaker's recording
 * alignable.  Lattice [t_x][t_y], path from (0, 0) to (t_x - 1, t_y - 1): D(0, 0) = c(0, 0), D(i, j) = c(i, j) + min(D(i-1, j-1), D(i-1, j),
 * D(i, j-1)) with +inf outside the lattice: a min and exactly one fp32 add per cell.  The predecessor is the argmin; ties go to the diagonal,
 * then to (i-1, j), then to (i, j-1).  NaN inputs are excepted.  Outputs per utterance, each optional: rows [B][Ty] (rows[j] = the largest i
 * on the path in column j; -1 for j >= t_y), cols [B][Tx] (cols[i] = the largest j on the path in row i; -1 for i >= t_x),
 * total [B] = D(t_x - 1, t_y - 1), steps [B] = the number of path cells.  A length > its capacity raises AS_STATUS_CAPACITY and is
 * clamped; a length <= 0 writes only the -1 fill (total and steps of that utterance are left alone).
 * as_dtw_f32            a caller's dense cost [B][Tx][Ty] (the counterpart of as_mas_f32), t_x / t_y DEVICE int32 [B].  Two launches (the lattice
 *                       re-laid in the order of the wavefront's steps, then the warp and the walk back).
 * as_dtw_features_f32   packed features [C][ld] on both sides; utterance u lies at the columns [mult off[u], mult off[u + 1]) of its side
 *                       (off DEVICE int32 [B + 1]; as_forward_io.mel_out lies at 2 * frame_off), cut at ld and at the capacity
 *                       (AS_STATUS_CAPACITY).  Four launches: the means and the spans, the cost lattice (into the workspace, or into cost_out
 *                       [B][Tx][Ty] if given; cells outside an utterance's lattice are not written), then as_dtw_f32's two.
 * as_transfer_rows_f32  one launch, a workgroup per utterance.  Packed token k of utterance u (tok_off DEVICE [B + 1]) owns the synthesised
 *                       columns [2 s_k, 2 s_{k+1}), s_k = pass A's dur_i summed over u's tokens before k.  E_k = the first j < t_y with
 *                       rows[j] >= 2 s_{k+1}, else t_y (t_y = the recording's span, cut at ld_rows); E_{-1} = 0; H_k = (E_k + 1) >> 1; the
 *                       target t_k = clamp(H_k - H_{k-1}, 1, 16384) goes to target_dur[k] (optional).  out_rows[k] (row stride ld_out >=
 *                       AS_PROSODY_DIM, columns behind AS_PROSODY_DIM are left alone): [AS_PROSODY_DUR] = q = fp32(t_k) / duration_k; if q is
 *                       not finite or rintf(fp32(duration_k q)) != t_k, q = 1 and misses[u] (optional, [B]) goes up; with strength[0] == 0 the
 *                       scale is 1 and nothing is a miss.  Gains 1.  [AS_PROSODY_OFFSET + c] = strength[1 + c] (mean_rec - mean_syn): mean_rec
 *                       over the columns [E_{k-1}, E_k) of row (c == 0 ? 1 : c == 1 ? 0 : c) of feat12 (as_ref_features_f32: energy, F0,
 *                       EMA), mean_syn over the token's own columns of pass A's F0 / N / EMA (as_forward_io.F0 ...; cut at the utterance's
 *                       span), both fp32 sums in ascending order / fp32(count); 0 if either range is empty.  Tokens from tok_cap on are not
 *                       written (AS_STATUS_CAPACITY).  The offsets are FIRST ORDER: measured against pass A's tracks, while pass B's
 *                       predictors see the new durations.  Durations go in as a scale because a plan with token rows refuses forced_dur.
 * as_dtw_host, as_dtw_features_host, as_transfer_rows_host: the same rule on HOST arrays (every pointer is a host pointer; no GPU, no
 *                       workspace, over-long lengths are clamped without a word).
 * AS_EINVAL before anything is launched: a NULL io, input, offset array or workspace, B < 1, a capacity outside [1, AS_DTW_MAX_T],
 * C outside [1, AS_DTW_MAX_C], a multiplier < 1, ld below what one frame needs (ld < 1; ld_out < AS_PROSODY_DIM), center not 0 or 1, a
 * negative or non-finite strength.  AS_ENOSPC: ws_bytes below as_dtw_workspace_bytes(B, Tx, Ty) (0 for arguments it refuses).  AS_EDEVICE
 * while a status bit is set. */
#define AS_DTW_MAX_T 4096
#define AS_DTW_MAX_C 128
typedef struct as_dtw_io {
    const float* a; int32_t lda; const int32_t* a_off; int32_t a_mult;    /* the synthesised side [C][lda] */
    const float* b; int32_t ldb; const int32_t* b_off; int32_t b_mult;    /* the recording [C][ldb] */
    int32_t C, B, Tx, Ty, center;
    int32_t* rows; int32_t* cols; float* total; int32_t* steps;           /* optional outputs */
    float* cost_out;                                                      /* optional [B][Tx][Ty] */
} as_dtw_io;
typedef struct as_transfer_io {
    int32_t B;
    const int32_t* rows; int32_t ld_rows;                                 /* the warp's rows [B][ld_rows] */
    const int32_t* tok_off; int32_t tok_cap;                              /* [B + 1]; the packed tokens there is room for */
    const int32_t* dur_i; const float* duration;                          /* pass A's, [sum tok_lens] */
    const float* F0; const float* N; const float* EMA; int32_t ld_pred;   /* pass A's tracks: [1] / [1] / [10] x [ld_pred] */
    const int32_t* syn_off; int32_t syn_mult;                             /* [B + 1]: utterance u at the columns syn_mult * syn_off[u] .. */
    const float* feat12; int32_t ld_feat;                                 /* the recording's tracks [12][ld_feat] */
    const int32_t* rec_off; int32_t rec_mult;                             /* [B + 1] */
    float strength[13];                                                   /* timing, then F0, N, EMA0..9 */
    float* out_rows; int32_t ld_out;                                      /* [tok_cap][ld_out >= AS_PROSODY_DIM] */
    int32_t* target_dur;                                                  /* optional [tok_cap] */
    int32_t* misses;                                                      /* optional [B] */
} as_transfer_io;
size_t as_dtw_workspace_bytes(int B, int Tx, int Ty);
int as_dtw_f32(const float* cost, const int32_t* t_x, const int32_t* t_y, int B, int Tx, int Ty, int32_t* rows, int32_t* cols,
               float* total, int32_t* steps, void* ws, size_t ws_bytes, as_stream_t stream);
int as_dtw_features_f32(const as_dtw_io* io, void* ws, size_t ws_bytes, as_stream_t stream);
int as_transfer_rows_f32(const as_transfer_io* io, as_stream_t stream);
int as_dtw_host(const float* cost, const int32_t* t_x, const int32_t* t_y, int B, int Tx, int Ty, int32_t* rows, int32_t* cols,
                float* total, int32_t* steps);
int as_dtw_features_host(const as_dtw_io* io);
int as_transfer_rows_host(const as_transfer_io* io);

/* ---- batches in flight (csrc/lanes.hip; DESIGN.md section 5: the throughput arrangement) -----------------------------------------------
 * as_lanes = n lanes on ONE model: per lane a HIP stream of its own, its two workspaces (grown on demand), TWO serial plans
 * (as_plan_set_serial) -- one for eager calls, whose layout cache may be flushed at any entry point, and one that only ever sees the
 * geometries that are replayed from hipGraphs and is reset only together with them -- and the hipGraphs of the (geometry, io) pairs it
 * has replayed.  as_lanes_submit enqueues ONE batch (ArtsSpeech.forward(step="test"), as as_forward_test) on the next lane, round robin,
 * and returns at once; before it does it waits until that lane's PREVIOUS batch has finished -- so the device buffers named by a lane's
 * as_forward_io may be refilled once the submit that follows them on the same lane has been entered, or after as_lanes_wait.  Fill a
 * lane's input buffers on ITS stream (as_lanes_stream(q, as_lanes_next(q))) or synchronise before submitting.  With batch->frames given
 * (forced durations, or a second pass) a (geometry, io) pair runs eagerly twice on a lane (first on the eager plan, then on the graph
 * plan, which uploads its tables), the third submit is captured into a hipGraph and later ones are one hipGraphLaunch; a lane keeps at
 * most as_lanes_set_graph_cap graphs (default 256) and drops them all -- with the graph plan's tables -- when one more is wanted.  With
 * frames == NULL (predicted durations) and no frame capacity every submit runs as_forward_test eagerly, which synchronises that lane's stream
 * once to read the frame counts, and a workspace too small for them is re-sized and the call repeated (AS_ENOSPC only if io->ld_out itself
 * is too small: frames_host_out then says what is needed); with io->frame_cap > 0 (as_forward_io: the durations stay on the device) such a
 * submission is eager, captured, replayed -- and coalesced -- like one with known counts.  A workspace that is outgrown is kept until as_lanes_wait(q, -1) / as_lanes_destroy (freeing
 * it would synchronise the device under the other lanes).  Not thread-safe: one host thread per as_lanes.  as_lanes_wait(q, lane):
 * lane < 0 = all; AS_EDEVICE if a kernel raised a status bit (as_device_status). */
typedef struct as_lanes as_lanes;
int as_lanes_create(const as_model* m, int n_lanes, as_lanes** out);
int as_lanes_destroy(as_lanes* q);
int as_lanes_count(const as_lanes* q);
int as_lanes_next(const as_lanes* q);
as_stream_t as_lanes_stream(const as_lanes* q, int lane);
int as_lanes_submit(as_lanes* q, const as_batch* batch, const as_forward_io* io, int32_t* frames_host_out, int32_t* lane_out);
int as_lanes_wait(as_lanes* q, int lane);
/* Coalescing (k > 1; 1 = off, the default).  Every tensor of the path concatenates the utterances along its column axis, so submissions
 * whose buffers are ADJACENT views of one block -- the next one's tokens / mel / f0_raw / ema_raw / forced_dur / mel_out begin exactly where
 * the previous one's end, with the same leading dimensions -- are one batch as they lie: a lane holds such a submission back (frames given,
 * no optional outputs; or a frame capacity, io->frame_cap: then only the INPUTS have to be adjacent, every submission keeps its own mel_out
 * and may ask for its own frame_off, as_segments) until k neighbours have arrived and launches them as ONE as_forward_test call, without a copy (wider conv GEMM
 * launches; one fetch of the weights for k batches).  A submission that is not the neighbour of what waits on its lane sends that group out
 * first; as_lanes_wait and as_lanes_flush launch whatever waits.  With k > 1 a submit may therefore return before anything of it is
 * enqueued, and the status of a group's launch is returned by the call that triggers it; the host arrays of as_batch are copied at
 * submit.  DEVICE BUFFERS with k > 1: a submission's buffers are read when its GROUP is launched, not when it is submitted, and entering
 * the next submit of a lane no longer means the lane's previous work has finished (that submit may only be queued): refill or reuse a
 * lane's buffers after as_lanes_wait(q, lane) -- or keep two blocks per lane and alternate.  Re-submitting the SAME unchanged buffers (a
 * benchmark's replay) needs nothing: a group's launch first waits for the lane's previous group.  The turn passes to the next lane when
 * a group is launched; as_lanes_destroy launches what still waits before it tears the lanes down.
 * (models.py:361-362 processes one utterance at a time: any grouping is legal, and every utterance gets its batch-1 result.)
 * Voice mode (as_forward_io.voices): the tokens (and forced_dur / mel_out as above) are adjacent and the voices continue each other -- both
 * with indices, the same voices / ld_voice / n_voices and voice_idx = the previous voice_idx + its B; or both without, the same ld_voice and
 * voices = the previous voices + its B * ld_voice.  A voice submission never joins a group of reference submissions, nor the reverse.  The
 * graph key holds the voice fields; the indices are device data read at replay.  Debug checksums cover voice_idx instead of the reference
 * rows.
 * Prosody control (as_forward_io.prosody): submissions join a group only if all of them carry rows with the same ld_prosody, each
 * submission's rows beginning where the previous one's end (prosody = the previous prosody + its B * ld_prosody), or none of them does.
 * The graph key holds prosody / ld_prosody; the rows are device data read at replay.  Debug checksums cover them. */
int as_lanes_set_coalesce(as_lanes* q, int k);
int as_lanes_flush(as_lanes* q);
/* Debug mode (also switched on by AS_DEBUG=1 in the environment at as_lanes_create).  The buffer rule above is the caller's to keep, and a
 * caller that breaks it corrupts a batch without a sign.  With debug on, the device inputs of a submission that is held back for its group
 * (tokens, forced durations, f0, the EMA and mel rows) are checksummed when it is submitted -- the submit then WAITS for its lane's stream, so
 * the sum is of what was handed over -- and again when the group is launched: a difference raises AS_STATUS_BAD_LAYOUT and the call that
 * launches the group returns AS_EDEVICE.  One stream synchronisation per submission: not for production traffic. */
int as_lanes_set_debug(as_lanes* q, int on);
/* Host submissions: the boundary of the reference hands over HOST arrays (test.py:96-113 moves tokens / mel to the device inside
 * `synthesis` and the mel back), and under coalescing the device-buffer rule above is easy to get wrong -- so the lane can own the device
 * side.  as_lanes_submit_host copies the submission's inputs into the next free column range of the lane's own device block (one block per
 * lane: a group's submissions lie side by side in it, i.e. they are adjacent as as_lanes_set_coalesce wants them, with no gather), launches
 * the group when it is full (coalesce = 1: at once) and copies every submission's mel to ITS host array behind the launch.  A lane keeps
 * TWO such blocks and alternates between them from group to group; the copies run on ONE pair of copy streams, one per direction, that all
 * lanes share: the copies of a lane's next group run under the kernels of its current one, and a block is refilled only behind the
 * kernels AND the result copies of the group that used it last (events between the lane's stream and the shared pair; nothing for the
 * caller to keep).  batch->frames is optional: given (forced durations, or known from an earlier pass), or NULL with frame_cap and
 * frame_off below (durations predicted on the device).  Pointers are HOST pointers: pinned memory (hipHostMalloc) for copies that do not
 * block the calling thread; the input arrays must stay unchanged and the output array is valid after as_lanes_wait(q, lane) (lane =
 * *lane_out) has returned.  Whether a submission joins what waits on its lane is decided by the rule of as_lanes_set_coalesce, applied to
 * its place in the block: one that does not fit behind the group there, is of the other kind (known frames / a capacity; forced durations
 * or none; another voice table; prosody or none) or follows a device submission sends that group out first.  Debug mode
 * (as_lanes_set_debug) does not cover host submissions: their device buffers are the lane's block, which only the library writes, so
 * there is nothing a caller could overwrite between submit and launch -- no checksum is taken and none is compared. */
typedef struct as_host_io {
    const int32_t* tokens;                 /* [sum tok_lens] */
    const float* mel; int32_t ld_mel;      /* [n_mels][ld_mel >= sum ref_lens] */
    const float* f0_raw;                   /* [sum ref_lens] */
    const float* ema_raw; int32_t ld_ema;  /* [10][ld_ema >= sum ref_lens] */
    const int32_t* forced_dur;             /* optional [sum tok_lens] */
    float* mel_out; int32_t ld_out;        /* [n_mels][ld_out >= 2 * sum frames] */
    /* predicted durations (batch->frames == NULL; as_forward_io.frame_cap): the half-rate frames there is room for, and where the
     * utterances' frame offsets [B + 1] go (HOST; required: it is how the caller finds its utterances in mel_out, whose row stride is then
     * ld_out >= 2 * frame_cap and which is copied back whole) */
    int32_t frame_cap;
    int32_t* frame_off;
    /* voice mode (as_forward_io.voices): voices is a DEVICE table [n_voices][ld_voice] that stays resident (it is not copied: keep it
     * unchanged until as_lanes_wait); voice_idx is HOST int32 [B] (or NULL = row b), copied into the lane's block like the tokens.  mel,
     * f0_raw, ema_raw and batch->ref_lens are then not read. */
    const float* voices; int32_t ld_voice, n_voices;
    const int32_t* voice_idx;
    /* prosody control (as_forward_io.prosody): HOST fp32 [B][ld_prosody >= AS_PROSODY_DIM], or NULL; its rows are copied into the lane's
     * block beside the tokens */
    const float* prosody; int32_t ld_prosody;
} as_host_io;
int as_lanes_submit_host(as_lanes* q, const as_batch* batch, const as_host_io* io, int32_t* lane_out);
int64_t as_lanes_merged_calls(const as_lanes* q, int lane);   /* as_forward_test calls of this lane that held more than one submission */
/* tuning / tests: graphs a lane keeps (>= 1), and the layout cap of every lane's eager plan (as_plan_set_layout_cap) */
int as_lanes_set_graph_cap(as_lanes* q, int max_graphs);
int as_lanes_set_layout_cap(as_lanes* q, int max_layouts);
/* every lane's workspaces A / B get at least this many bytes now: a server that knows its largest batch (as_module_workspace_bytes) never
 * re-sizes a workspace -- which would drop that lane's graphs -- in the middle of traffic */
int as_lanes_reserve(as_lanes* q, size_t bytes_a, size_t bytes_b);
/* counters of lane `lane`: [0] graphs held, [1] times all graphs were dropped, [2] layout flushes of the eager plan, [3] graph launches,
 * [4] eager calls, [5] captures */
int as_lanes_stats(const as_lanes* q, int lane, int64_t* out6);

#ifdef __cplusplus
}
#endif
#endif /* ARTSPEECH_HIP_H */
