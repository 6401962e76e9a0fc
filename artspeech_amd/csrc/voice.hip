// Voice mode of as_forward_test (include/artspeech_hip.h: as_forward_io.voices): the per-utterance gather of a precomputed voice.
//
// A voice row holds Style [n_style] then dur_style [n_dur] (as_voice_forward's layout).  Utterance b reads row idx[b] (idx NULL: row b)
// and writes its Style row and its dur_style row where the forward's first half keeps them.  An index outside [0, n_voices) writes zeros
// -- nothing outside the table is read -- and raises AS_STATUS_BAD_VOICE: the utterance's result is void and every later module call
// returns AS_EDEVICE until the bit is cleared.  The indices are device data read when the kernel runs, so a replayed hipGraph sees
// whatever the caller wrote into them since.
#include "common.h"
#include "artspeech_hip.h"

namespace {

__global__ void __launch_bounds__(256)
voice_gather_kernel(const float* __restrict__ voices, int ld_voice, int n_voices, const int32_t* __restrict__ idx, int n_style, int n_dur,
                    float* __restrict__ style, int ld_style, float* __restrict__ ds, int ld_ds, unsigned* status)
{
    const int b = blockIdx.x;
    const int v = idx ? idx[b] : b;
    const bool ok = v >= 0 && v < n_voices;
    if (!ok && threadIdx.x == 0) as_status_raise(status, AS_STATUS_BAD_VOICE);
    const float* row = voices + (size_t)(ok ? v : 0) * ld_voice;
    for (int i = threadIdx.x; i < n_style + n_dur; i += blockDim.x) {
        const float x = ok ? row[i] : 0.f;
        if (i < n_style) style[(size_t)b * ld_style + i] = x;
        else ds[(size_t)b * ld_ds + (i - n_style)] = x;
    }
}

}  // namespace

int as_voice_gather_launch(const float* voices, int ld_voice, int n_voices, const int32_t* idx, int B, int n_style, int n_dur, float* style,
                           int ld_style, float* ds, int ld_ds, hipStream_t stream)
{
    if (!voices || !style || !ds || B < 1 || n_voices < 1 || n_style < 1 || n_dur < 0 || ld_voice < n_style + n_dur || ld_style < n_style ||
        ld_ds < n_dur)
        return AS_EINVAL;
    AsProfScope prof(AS_CLS_OTHER, 0.0, 4.0 * B * (double)(2 * (n_style + n_dur) + 1), stream, "voice_gather");
    hipLaunchKernelGGL(voice_gather_kernel, dim3(B), dim3(256), 0, stream, voices, ld_voice, n_voices, idx, n_style, n_dur, style, ld_style, ds,
                       ld_ds, as_status_words_device());
    AS_CHECK_LAUNCH();
    return AS_OK;
}
