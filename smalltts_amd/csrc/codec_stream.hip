// Streamed codec decode (DESIGN '8f. Streamed decode'), gfx950: carry_frames, the one kernel a chunked decode adds.
//
// Every codec image is channels-last [B][8 + T][C] with 8 pad frames in front of each row (kCodecPad, engine.hpp); the kernels that
// look back in time (k = 7 convs: 6 frames, ConvTranspose: 1 frame) read those pad frames from memory like any other frame.  A chunk
// therefore decodes exactly like the middle of a long utterance once the pad frames of a consumer's input hold the last 8 frames that
// image had in the previous chunk.  carry_frames does that for one image ("boundary"): with S the boundary's [8][C] block in the
// stream's state slot and X the T data frames of this chunk, for j in 0..7
//     pad[j]   <- S[j]
//     S_new[j] <- X[T - 8 + j]   where T - 8 + j >= 0,   S[j + T] otherwise (T < 8: the state moves up by T, the chunk enters behind it)
// A zero block is the start of an utterance (the causal zeros).  Pure copies of bits.
//
// A thread owns the 4 channels [4 g, 4 g + 4) of one batch row for all 8 j: 16 loads of 16 bytes (the 8 old state frames, the 8 frames
// of the new state), THEN 16 stores of 16 bytes.  S and S_new are the same memory; since a thread has read everything it will ever read
// before its first store, and no other thread touches its channels of its slot (a slot appears once per call), the update is in place
// without a barrier, an atomic or a second buffer.  One launch per boundary whatever B is; nothing outside the 8 pad frames and the last
// min(T, 8) data frames of each row of the image and the boundary's block of each listed slot is read, nothing outside the pad frames
// and that block is written.  Launch-bound (a boundary of the default spec moves at most B x 4 x 64 KB): plain C++.
#include "kernels.hpp"
#include "prof.hpp"

namespace {

constexpr int CF_PAD = 8;   // kCodecPad
typedef float f32x4 __attribute__((ext_vector_type(4)));   // one 16-byte lane, held in registers

__global__ __launch_bounds__(256) void carry_frames_kernel(float* __restrict__ img, int B, int T, int C4, char* pool, long slot_stride,
                                                           long offset, long n_slots, const int64_t* __restrict__ slots) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * C4) return;
    const int b = (int)(i / C4), g = (int)(i % C4);
    long s = (long)slots[b];
    s = s < 0 ? 0 : s >= n_slots ? n_slots - 1 : s;   // the table lives on the device: an index out of range is clamped, not followed
    f32x4* const S = reinterpret_cast<f32x4*>(pool + s * slot_stride + offset) + g;          // frame j: S[j * C4]
    f32x4* const row = reinterpret_cast<f32x4*>(img) + (long)b * (CF_PAD + T) * C4 + g;      // pad frame j: row[j * C4]
    f32x4 old[CF_PAD], nw[CF_PAD];
#pragma unroll
    for (int j = 0; j < CF_PAD; ++j) old[j] = S[(long)j * C4];
#pragma unroll
    for (int j = 0; j < CF_PAD; ++j) {
        const int t = T - CF_PAD + j;
        const f32x4* const src = t >= 0 ? row + (long)(CF_PAD + t) * C4 : S + (long)(j + T) * C4;
        nw[j] = *src;
    }
#pragma unroll
    for (int j = 0; j < CF_PAD; ++j) row[(long)j * C4] = old[j];
#pragma unroll
    for (int j = 0; j < CF_PAD; ++j) S[(long)j * C4] = nw[j];
}

}  // namespace

hipError_t launch_carry_frames(float* img, int B, int T, int C, void* pool, long slot_stride, long offset, long n_slots,
                               const int64_t* slots, hipStream_t st) {
    if (B < 1 || T < 1 || C < 4 || C % 4 || n_slots < 1 || offset < 0 || slot_stride < offset + (long)CF_PAD * C * 4 || !img || !pool ||
        !slots)
        return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(img) | reinterpret_cast<uintptr_t>(pool) | (uintptr_t)slot_stride | (uintptr_t)offset) & 15)
        return hipErrorInvalidValue;   // 16-byte lanes
    const long n = (long)B * (C / 4);
    ProfScope ps(st, "carry_frames", 0.0, 4.0 * CF_PAD * 4.0 * B * C);
    hipLaunchKernelGGL(carry_frames_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, img, B, T, C / 4,
                       static_cast<char*>(pool), slot_stride, offset, n_slots, slots);
    return hipGetLastError();
}
