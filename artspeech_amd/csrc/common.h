// Shared helpers for the gfx950 kernels behind include/artspeech_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define AS_OK 0
#define AS_EINVAL (-1)
#ifndef AS_EDEVICE
#define AS_EDEVICE (-3)
#endif

// device-side status words (status.hip; kinds in include/artspeech_hip.h)
unsigned* as_status_words_device();     // device address of the current device's words, or NULL
int as_status_peek();                   // host view: bit k = kind k raised

// Launch-error check: returns the hipError_t (>0) from the calling extern "C" function.
#define AS_CHECK_LAUNCH()                        \
    do {                                         \
        hipError_t e__ = hipGetLastError();      \
        if (e__ != hipSuccess) return (int)e__;  \
    } while (0)

#define AS_CHECK(call)                           \
    do {                                         \
        hipError_t e__ = (call);                 \
        if (e__ != hipSuccess) return (int)e__;  \
    } while (0)

static inline int as_cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// The opt-in for more than 64 KiB of dynamic LDS is a per-device function attribute: one of these per call site sets it once on every
// device the process drives (the library keeps per-device state elsewhere too: status.hip), from any host thread.
struct AsLdsOptIn {
    unsigned long long done = 0;        // bit d: set on device d (read / written with __atomic builtins)
    int ensure(const void* fn, int bytes)
    {
        int d = 0;
        hipError_t e = hipGetDevice(&d);
        if (e != hipSuccess) return (int)e;
        const unsigned long long bit = 1ull << (d & 63);
        if (__atomic_load_n(&done, __ATOMIC_ACQUIRE) & bit) return AS_OK;
        e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e != hipSuccess) return (int)e;
        __atomic_fetch_or(&done, bit, __ATOMIC_RELEASE);
        return AS_OK;
    }
};
#define AS_LDS_OPT_IN(fn, bytes)                                                   \
    do {                                                                           \
        static AsLdsOptIn opt__;                                                   \
        const int r__ = opt__.ensure(reinterpret_cast<const void*>(fn), (bytes));  \
        if (r__ != AS_OK) return r__;                                              \
    } while (0)

#define AS_WAVE 64

// Capacity layouts of as_forward_test's second half (as_forward_io.frame_cap; csrc/model.hip "dynamic layouts", elementwise.hip): the
// utterances' frame counts exist on the device only -- frame_off [B + 1], half rate, packed from column 0 -- and every table the kernels of
// the second half read is derived from them by ONE launch.  Layout i of {0: half rate, 1: mel rate, 2: the batch three times at half rate
// (group g from column g * cap1), 3: the same at mel rate}: widths w[i], first columns off[i] (one closing entry), column descriptors
// meta[i], *nvalid[i] = the valid leading columns (of a group).  Any pointer may be NULL.
struct AsDynGeo {
    const int32_t* frame_off;
    int32_t B, cap1, n_seg;
    int32_t seg_first[17];            // segments = the submissions of a merged call: utterances [seg_first[s], seg_first[s + 1])
    int32_t seg_cap[16];              // ... and the half-rate frames the segment's output slot holds
    int32_t* seg_frame_off[16];       // optional: the segment's own frame offsets [its utterances + 1], from 0
    int32_t* w[4];
    int32_t* off[4];
    unsigned long long* meta[4];
    int32_t* nvalid[4];
    int32_t* src3;                    // [3 B]: where utterance b of group g reads the shared half-rate input (= off[0][b])
    int32_t* tof;                     // frame -> token map [cap1]: entries past the last frame are set to token 0
    unsigned* status;
};
int as_dyn_geometry_launch(const AsDynGeo& g, hipStream_t stream);
// mel [rows][ld_src] packed from column 0 -> every segment's columns to its own slot of dst: dst_s[r][i] = src[r][2 off[first_s] + i]
struct AsSegScatter {
    const float* src; int32_t ld_src, rows, n_seg;
    const int32_t* frame_off;
    int32_t seg_first[17];
    int32_t seg_cap[16];
    float* dst[16]; int32_t ld_dst[16];
};
int as_seg_scatter_launch(const AsSegScatter& a, hipStream_t stream);
// voice mode (voice.hip): utterance b's Style [n_style] and dur_style [n_dur] from row idx[b] (NULL: b) of voices [n_voices][ld_voice];
// an index outside [0, n_voices) writes zeros and raises AS_STATUS_BAD_VOICE
int as_voice_gather_launch(const float* voices, int ld_voice, int n_voices, const int32_t* idx, int B, int n_style, int n_dur, float* style,
                           int ld_style, float* ds, int ld_ds, hipStream_t stream);
// prosody control (as_forward_io.prosody, rows [B][ld_pros >= AS_PROSODY_DIM]; elementwise.hip).  as_durations_f32 with every predicted
// duration of utterance b multiplied by pros[b][AS_PROSODY_DUR] before it is rounded (pros NULL: as_durations_f32 itself)
int as_durations_prosody_launch(const float* dur_f32, const int32_t* forced_dur, const int32_t* tok_off, int B, const float* pros, int ld_pros,
                                int32_t* dur_i32, int32_t* frame_off, int32_t* tok_of_frame, int max_frames, hipStream_t stream);
// as_project_cols_f32 whose output row m is track track0 + m: column j of utterance b (col_off [B + 1], device) is stored as
// fmaf(gain[b][track], y, offset[b][track]); columns at or past col_off[B] (a capacity layout's filler) as computed
int as_project_cols_prosody_launch(const float* x, int ldx, int K, int N, const float* w, const float* bias, int M, float* y, int ldy,
                                   const float* pros, int ld_pros, const int32_t* col_off, int B, int track0, hipStream_t s);
// per-token prosody (as_plan_set_token_prosody, rows [ntok][ld >= AS_PROSODY_DIM]; token_prosody.hip, the rule: token_prosody.h).
// out[i] = dur_f32[i] * rows[i][AS_PROSODY_DUR] (* pros[utterance of i][AS_PROSODY_DUR] when pros is given): what the durations launch
// then reads in place of the predictor's output
int as_token_dur_scale_launch(const float* dur_f32, const float* rows, int ld, const int32_t* tok_off, int B, int ntok, const float* pros,
                              int ld_pros, float* out, hipStream_t stream);
// start [ntok + 1] = the exclusive prefix sum of the integer durations over the packed tokens (half-rate frames)
int as_token_starts_launch(const int32_t* dur_i32, int ntok, int32_t* start, hipStream_t stream);
// every value of the valid full-rate columns of fne [12][ld] (n_cols = 2 n_frames_max of them; valid: below 2 frame_off[B]) becomes
// fmaf(gain, x, offset) with its column's gains and offsets by token_prosody.h's rule; tof [n_frames_max] = the frame -> token map
int as_token_tracks_launch(float* fne, int ld, int n_cols, const int32_t* tof, int n_frames_max, const int32_t* frame_off, const int32_t* tok_off,
                           int B, int ntok, const int32_t* start, const float* rows, int ld_rows, int smooth, hipStream_t stream);
// fit to time (as_plan_set_fit; duration_fit.hip, the rule: duration_fit.h).  as_fit_durations_f32 on v[i] * pros[utterance of i]
// [AS_PROSODY_DUR] (pros NULL: on v itself): dur_i [ntok] for every token, the spans' tokens fitted; ws: as_fit_workspace_bytes
struct as_fit;
bool as_fit_valid(const as_fit* fit);
int as_fit_launch(const float* v, const float* pros, int ld_pros, const int32_t* tok_off, int B, int ntok, const as_fit& fit, int32_t* dur_i,
                  int32_t* span_scale_q16, void* ws, hipStream_t stream);

// fp32 samples w [N] -> 16-bit PCM by the rule of as_conv_post_pcm_f32 (vocoder.hip; a NaN stores 0 and raises AS_STATUS_F16_RANGE).
// n_valid (a capacity layout, device count): samples [*n_valid, N) are not read; pcm and w_fill (each may then be NULL) get 0 there
int as_pcm16_launch(const float* w, int N, const int32_t* n_valid, float* w_fill, int16_t* pcm, hipStream_t stream);

// Capacity layouts of the HiFi-GAN generator (as_vocoder_forward_cap; vocoder.hip): the utterances' lengths exist on the device only --
// off [B + 1] in units of `mult` mel frames, packed from column 0 -- and ONE launch derives the tables of the mel-rate layout and of every
// up-sampled one (rate[i] columns per mel frame, rate[0] = 1) from them.  The tables are two flat arrays:
//   tab  int32 [n_rates][2 B + 2]: per rate the widths w [B], the first columns off_r [B + 1], then n_valid (= off_r[B])
//   meta [cap * sum rate]:         rate i's column descriptors start at cap * (rate[0] + ... + rate[i - 1])
// Offsets are cut at cap (AS_STATUS_CAPACITY when off[B] * mult > cap, or when an utterance has more than max_len mel frames); an
// utterance wider than AS_META_MAX_W columns at a rate raises AS_STATUS_BAD_LAYOUT and its columns there get one-column descriptors.
#define AS_VOC_MAX_RATES 9
struct AsVocGeo {
    const int32_t* off;
    int32_t B, mult, cap, max_len, n_rates;
    int32_t rate[AS_VOC_MAX_RATES];
    long long meta_start[AS_VOC_MAX_RATES];   // in descriptors
    int32_t* tab;
    unsigned long long* meta;
    int32_t* sample_off;                      // optional [B + 1]: off_r of the last rate
    unsigned* status;
};
int as_vocoder_cap_geometry_launch(const AsVocGeo& g, hipStream_t stream);

// Windowed vocoding (window.hip; the rule: window_rule.h): as_window_gather_f32 / as_window_stitch_f32 with the look at the device status
// as an option (peek false: inside as_vocoder_forward_windowed, which has looked once)
struct as_window_cfg;
int as_window_gather_launch(const as_window_cfg* w, int round, const float* mel, int ld_mel, int num_mels, const int32_t* off, int B, int mult,
                            int cap, int max_len, float* wmel, int ld_w, int32_t* woff, int32_t* skip_count, bool peek, hipStream_t s);
int as_window_stitch_launch(const as_window_cfg* w, int round, const float* wwav, int ld_w, const int32_t* woff, const int32_t* off, int B,
                            int mult, int cap, int max_len, float* wav, int16_t* pcm, int32_t* sample_off, bool peek, hipStream_t s);

// kernel classes for the optional event profiler (prof.hip)
enum { AS_CLS_GEMM = 0, AS_CLS_ADAIN = 1, AS_CLS_LN = 2, AS_CLS_ATTN = 3, AS_CLS_LSTM = 4, AS_CLS_MAS = 5, AS_CLS_OTHER = 6, AS_N_CLS = 7 };
struct AsProfScope {
    int idx;
    hipStream_t stream;
    AsProfScope(int cls, double flops, double bytes, hipStream_t s, const char* tag = nullptr);
    ~AsProfScope();
};

#ifdef __HIPCC__
// raise status kind `kind` (a kernel's failure path only): one system-scope store into pinned host memory
static __device__ __forceinline__ void as_status_raise(unsigned* words, int kind)
{
    if (words) __hip_atomic_store(words + kind, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// the waveform as 16-bit PCM (include/artspeech_hip.h, as_conv_post_pcm_f32; vocoder.hip, resample.hip): one fp32 multiply, round half to even, saturate; a NaN gives 0
// (*nan says so: the caller raises AS_STATUS_F16_RANGE)
static __device__ __forceinline__ int as_pcm16(float w, bool* nan)
{
    *nan = w != w;
    return *nan ? 0 : (int)fmaxf(-32768.f, fminf(32767.f, rintf(__fmul_rn(32767.f, w))));
}
// 64-lane butterfly sum / maximum, o = 32 .. 1: every lane gets the result, and every kernel that must agree bitwise uses this one order
template <typename T>
static __device__ __forceinline__ T as_wave_sum(T v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
static __device__ __forceinline__ float as_wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
// THE ORDER OF ADDITIONS of the AdaIN statistics over an utterance of L columns (adain_kernel, adain_image_kernel, the K-sliced
// reduction with the AdaIN behind it: the same bits in all of them): one wave per channel, a lane adds its elements i = lane, lane + 64,
// ... in ascending order, then as_wave_sum; mean = sum / L; the variance is a second pass over d = __fsub_rn(x, mean) with
// __fmaf_rn(d, d, acc) per element, the same two steps; rstd = 1 / sqrtf(var / L + 1e-5f).
// AdaIN1d value and the fused depthwise ConvTranspose1d(k3, s2, p1, op1) pair, written with explicit roundings so that every
// kernel that evaluates them (adain_kernel: fp32 output; adain_image_kernel: operand image) produces the same bits whatever
// the compiler would contract.
static __device__ __forceinline__ float as_adain_val(float x, float mean, float rstd, float one_plus_gamma, float beta, int lrelu)
{
    const float o = __fmaf_rn(one_plus_gamma, __fmul_rn(__fsub_rn(x, mean), rstd), beta);
    return (lrelu && o < 0.f) ? __fmul_rn(0.2f, o) : o;
}
// out[2i] = a[i] w1 + b ; out[2i+1] = a[i] w2 + a[i+1] w0 + b
static __device__ __forceinline__ void as_convt_pair(float a0, float a1, float w0, float w1, float w2, float pb, float* o0, float* o1)
{
    *o0 = __fmaf_rn(a0, w1, pb);
    *o1 = __fadd_rn(__fmaf_rn(a1, w0, __fmul_rn(a0, w2)), pb);
}
#endif
