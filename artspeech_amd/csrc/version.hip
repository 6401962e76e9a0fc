#include "common.h"
#include "artspeech_hip.h"
// 8: ConvGemmArgs.slab_tr and as_conv_gemm_multi_post_f32's post_ln argument (round 5: assigned late), AsAdainArgs.col_w, as_forward_io's
// frame capacity, the host submissions and the debug checks of as_lanes (round 6)
// 9: voices -- as_voice_dim / as_voice_forward, as_forward_io and as_host_io voice fields, AS_MOD_VOICE / AS_MOD_FORWARD_A_VOICE,
// AS_STATUS_BAD_VOICE
// 10: prosody control -- as_forward_io and as_host_io prosody / ld_prosody, AS_PROSODY_DIM and the row offsets
// (10 still: as_plan_set_token_prosody and as_token_prosody came as a new entry point and a new struct -- no signature and no struct
// layout that existed changed, so a caller built against the earlier header goes on unchanged)
extern "C" int as_abi_version(void) { return AS_ABI_VERSION; }
