// decode_src.hip — decode_kernel<0, false, true>, the one-kernel front end that leaves the raw dynamic-range words for a
// transcode in source mode (ac3mi_set_encode_drc_source 1 under ac3mi_set_decode_mode 1, or mode 3 with a downmix), in a
// translation unit of its own.  Instantiated beside decode_kernel<0> in decode.hip it changes what the inliner does with the
// helpers the two then share, and decode_kernel<0> - which runs with the feature off - goes from 56 to 60 bytes of scratch.
// The parse kernels' SRC instantiations (MODE 4 / 5) leave their twins' figures alone and stay in decode.hip.
#undef DEC_STAMPS               // (the section timers' counters are decode.hip's)
#include "decode_kernel.h"

namespace ac3mi {

void launch_decode0_src(const DecodeParams &P, unsigned n_streams, size_t fr_bytes, hipStream_t stream)
{
    hipLaunchKernelGGL((decode_kernel<0, false, true>), dim3(n_streams), dim3(64), fr_bytes, stream, P);
}

}  // namespace ac3mi
