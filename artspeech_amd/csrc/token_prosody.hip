// Per-token prosody of as_forward_test (include/artspeech_hip.h: as_plan_set_token_prosody): rate, pitch, energy and articulators of
// single tokens inside an utterance.  Three small launches, made only by a forward whose plan has token controls set (csrc/model.hip):
//
//   token_dur_scale_kernel   one thread per packed token: the predictor's duration times the token's scale (and the utterance's, when
//                            as_forward_io.prosody is set too) into a workspace buffer that the durations kernel then rounds and clamps
//                            in place of the predictor's output;
//   token_starts_kernel      the exclusive prefix sum of the integer durations over the packed tokens, start[ntok + 1] (one workgroup;
//                            a thread owns a chunk of tokens, as in the durations kernel: a batch may hold more than 1 024 tokens);
//   token_tracks_kernel      one thread per full-rate column of the track buffer fne [12][ld] (F0, N, EMA0..9), behind the articulatory
//                            predictors and in front of the decoder: the column's token comes from the frame -> token map, its
//                            utterance's first and last token from a binary search in the token offsets, its control points and their
//                            weight from token_prosody.h's rule, and the twelve values of the column become fmaf(gain, x, offset) in
//                            place.  Row reads and stores are coalesced; the 25-float parameter rows of neighbouring columns are the
//                            same one or two rows and stay in cache.
// Columns at or past 2 * frame_off[B] (a capacity layout's filler) are not touched and their map entries are not read.  The parameter
// rows are device data read when the kernels run: a replayed hipGraph sees new contents.
#include "common.h"
#include "artspeech_hip.h"
#include "token_prosody.h"

#define AS_FILE_CLS AS_CLS_OTHER

namespace {

// the utterance of packed token i: the last b < B with tok_off[b] <= i (empty utterances share their offset with the one behind them,
// which this picks)
__device__ __forceinline__ int utterance_of(const int* __restrict__ tok_off, int B, int i)
{
    int lo = 0, hi = B - 1;
    while (hi > lo) {
        const int mid = (lo + hi + 1) >> 1;
        if (tok_off[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ void __launch_bounds__(256)
token_dur_scale_kernel(const float* __restrict__ dur_f, const float* __restrict__ rows, int ld, const int* __restrict__ tok_off, int B, int ntok,
                       const float* __restrict__ pros, int ldp, float* __restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= ntok) return;
    const float us = pros ? pros[(size_t)utterance_of(tok_off, B, i) * ldp + token_prosody::DUR] : 1.f;
    out[i] = token_prosody::scale_duration(dur_f[i], rows[(size_t)i * ld + token_prosody::DUR], pros != nullptr, us);
}

__global__ void __launch_bounds__(1024)
token_starts_kernel(const int* __restrict__ dur_i, int ntok, int* __restrict__ start)
{
    __shared__ int sums[1024];
    const int t = threadIdx.x;
    const int per = (ntok + 1023) / 1024, lo = min(t * per, ntok), hi = min(lo + per, ntok);
    int local = 0;
    for (int i = lo; i < hi; ++i) local += dur_i[i];
    sums[t] = local;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {             // inclusive scan of the chunk sums
        const int v = t >= off ? sums[t - off] : 0;
        __syncthreads();
        sums[t] += v;
        __syncthreads();
    }
    int f = sums[t] - local;                               // first frame of this thread's first token
    for (int i = lo; i < hi; ++i) {
        start[i] = f;
        f += dur_i[i];
    }
    if (t == 1023) start[ntok] = sums[1023];
}

__global__ void __launch_bounds__(256)
token_tracks_kernel(float* __restrict__ fne, int ld, int n_cols, const int* __restrict__ tof, int n_frames_max, const int* __restrict__ frame_off,
                    const int* __restrict__ tok_off, int B, int ntok, const int* __restrict__ start, const float* __restrict__ rows, int ldr,
                    int smooth)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int frames = min(frame_off[B], n_frames_max);     // (more frames than room: the layout was cut at the capacity)
    if (j >= n_cols || (j >> 1) >= frames) return;
    const int k = min(max(tof[j >> 1], 0), ntok - 1);
    const int u = utterance_of(tok_off, B, k);
    const token_prosody::Pick p = token_prosody::pick(smooth, j, k, tok_off[u], tok_off[u + 1] - 1, start);
#pragma unroll
    for (int m = 0; m < token_prosody::TRACKS; ++m) {
        const float g = token_prosody::param(p, rows, ldr, token_prosody::GAIN + m);
        const float o = token_prosody::param(p, rows, ldr, token_prosody::OFFSET + m);
        float* x = fne + (size_t)m * ld + j;
        *x = token_prosody::apply(g, *x, o);
    }
}

}  // namespace

int as_token_dur_scale_launch(const float* dur_f32, const float* rows, int ld, const int32_t* tok_off, int B, int ntok, const float* pros,
                              int ld_pros, float* out, hipStream_t stream)
{
    if (!dur_f32 || !rows || !tok_off || !out || ld < AS_PROSODY_DIM || B < 1 || B > 1024 || ntok < 0 || (pros && ld_pros < AS_PROSODY_DIM))
        return AS_EINVAL;
    if (ntok == 0) return AS_OK;
    AsProfScope prof__(AS_FILE_CLS, 2.0 * ntok, 12.0 * ntok, stream, "token_dur_scale");
    hipLaunchKernelGGL(token_dur_scale_kernel, dim3(as_cdiv(ntok, 256)), dim3(256), 0, stream, dur_f32, rows, ld, tok_off, B, ntok, pros, ld_pros, out);
    AS_CHECK_LAUNCH();
    return AS_OK;
}

int as_token_starts_launch(const int32_t* dur_i32, int ntok, int32_t* start, hipStream_t stream)
{
    if (!dur_i32 || !start || ntok < 0) return AS_EINVAL;
    AsProfScope prof__(AS_FILE_CLS, 0, 8.0 * ntok, stream, "token_starts");
    hipLaunchKernelGGL(token_starts_kernel, dim3(1), dim3(1024), 0, stream, dur_i32, ntok, start);
    AS_CHECK_LAUNCH();
    return AS_OK;
}

int as_token_tracks_launch(float* fne, int ld, int n_cols, const int32_t* tof, int n_frames_max, const int32_t* frame_off, const int32_t* tok_off,
                           int B, int ntok, const int32_t* start, const float* rows, int ld_rows, int smooth, hipStream_t stream)
{
    if (!fne || !tof || !frame_off || !tok_off || !start || !rows || ld < n_cols || n_cols < 0 || n_frames_max < 0 || n_cols > 2 * (long)n_frames_max ||
        B < 1 || B > 1024 || ntok < 0 || ld_rows < AS_PROSODY_DIM || (smooth != 0 && smooth != 1))
        return AS_EINVAL;
    if (n_cols == 0 || ntok == 0) return AS_OK;
    AsProfScope prof__(AS_FILE_CLS, 2.0 * AS_PROSODY_TRACKS * (double)n_cols, 8.0 * AS_PROSODY_TRACKS * (double)n_cols, stream, "token_tracks");
    hipLaunchKernelGGL(token_tracks_kernel, dim3(as_cdiv(n_cols, 256)), dim3(256), 0, stream, fne, ld, n_cols, tof, n_frames_max, frame_off, tok_off,
                       B, ntok, start, rows, ld_rows, smooth);
    AS_CHECK_LAUNCH();
    return AS_OK;
}
