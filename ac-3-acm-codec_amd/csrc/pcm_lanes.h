// pcm_lanes.h — the frame that the tools on s16 PCM in device memory share (loudness.hip, truepeak.hip, limit.hip): one
// wavefront per stream, a frame of 1536 instants as 64 segments of PCM_SEG = 24, one per lane, the lane's 24 NCH samples two
// to a dword.  Device parts are __forceinline__, without state and without LDS; the host parts are what every tool's
// launcher repeats: the channel count as a template constant, the roles of a call, one stream (or one wavefront) per grid slot.
// A tool writes its own params block, its per-frame work on the dwords and its state hand-over; truepeak_packed.h adds the
// interpolator's input for the tools that need the samples between the samples.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

namespace ac3mi {

constexpr int PCM_SEG = 24;             // sample instants of a lane's segment: 1536 / 64

// the stream of this wavefront, wave-uniform, in a kernel of `waves` wavefronts per workgroup (the caller leaves if it is none)
__device__ __forceinline__ unsigned pcm_wave_stream(int waves)
{
    return (unsigned)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * waves + (threadIdx.x >> 6)));
}

// The lane's 24 instants, 48 NCH contiguous bytes at fp, into w[12 NCH]: 16-byte loads where the call's base is 16-byte
// aligned (VEC: every frame and every lane's segment then is, 3072 and 48 NCH bytes apart), else 16-bit loads into the same
// registers - the same bits either way.  No sample is read twice
template <int NCH, bool VEC>
__device__ __forceinline__ void pcm_load_segment(const int16_t *fp, uint32_t *w)
{
    if constexpr (VEC) {
        const uint4 *v = reinterpret_cast<const uint4 *>(fp);
#pragma unroll
        for (int k = 0; k < 3 * NCH; k++) {
            const uint4 t = v[k];
            w[4 * k] = t.x; w[4 * k + 1] = t.y; w[4 * k + 2] = t.z; w[4 * k + 3] = t.w;
        }
    } else {
        const uint16_t *h = reinterpret_cast<const uint16_t *>(fp);
#pragma unroll
        for (int k = 0; k < 12 * NCH; k++) w[k] = (uint32_t)h[2 * k] | ((uint32_t)h[2 * k + 1] << 16);
    }
}

// ... and back: z[12 NCH] to the 48 NCH bytes at op
template <int NCH, bool VEC>
__device__ __forceinline__ void pcm_store_segment(int16_t *op, const uint32_t *z)
{
    if constexpr (VEC) {
        uint4 *v = reinterpret_cast<uint4 *>(op);
#pragma unroll
        for (int k = 0; k < 3 * NCH; k++) v[k] = make_uint4(z[4 * k], z[4 * k + 1], z[4 * k + 2], z[4 * k + 3]);
    } else {
        uint16_t *h = reinterpret_cast<uint16_t *>(op);
#pragma unroll
        for (int k = 0; k < 12 * NCH; k++) {
            h[2 * k] = (uint16_t)z[k];
            h[2 * k + 1] = (uint16_t)(z[k] >> 16);
        }
    }
}

// sample (instant i, slot c) of dwords that hold [instant][NCH] int16 from instant 0 on
template <int NCH>
__device__ __forceinline__ int32_t pcm_sample(const uint32_t *w, int i, int c)
{
    const int idx = i * NCH + c;
    return (int32_t)(int16_t)(w[idx >> 1] >> (16 * (idx & 1)));
}

// f(std::integral_constant<int, c>) for every slot c < NCH whose role is not 0, in order (a recursion: the slot is a
// compile-time constant in f, so the dwords it picks stay in registers)
template <int NCH, int C = 0, class F>
__device__ __forceinline__ void pcm_for_each_slot(const uint8_t *role, const F &f)
{
    if constexpr (C < NCH) {
        if (role[C] != 0) f(std::integral_constant<int, C>{});
        pcm_for_each_slot<NCH, C + 1>(role, f);
    }
}

// f(std::integral_constant<int, channels>) for the 1..6 channels that the tools' argument rules let through
template <class F>
inline void pcm_dispatch_channels(int channels, const F &f)
{
    switch (channels) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    default: f(std::integral_constant<int, 6>{}); break;
    }
}

// a call's roles in a block of N: the caller's for its channels (none given: 0), 0 behind them
template <int N>
inline void pcm_copy_roles(uint8_t (&dst)[N], const uint8_t *role, int channels)
{
    for (int c = 0; c < N; c++) dst[c] = role && c < channels ? role[c] : 0;
}

// `kernel` over n_streams streams, `per_block` of them to a workgroup of `threads` (a wavefront each: threads = 64 per_block;
// a lane each: threads = per_block)
template <class K, class... A>
inline hipError_t pcm_launch_streams(K kernel, int n_streams, int per_block, int threads, hipStream_t stream, const A &...args)
{
    if (n_streams <= 0) return hipSuccess;
    hipLaunchKernelGGL(kernel, dim3(((unsigned)n_streams + per_block - 1) / per_block), dim3(threads), 0, stream, args...);
    return hipGetLastError();
}

}  // namespace ac3mi
