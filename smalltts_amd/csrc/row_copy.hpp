// Row gathers of takes.hip and repair.hip: a workgroup grid (chunks, rows) copies whole rows of small buffers bit for bit, and the
// xor-butterfly wave sum both units count with.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

struct RowCopy {   // one copied buffer: rows of `n4` 4-byte elements; vec: 16-byte lanes (n4 % 4 == 0, both bases 16-byte aligned)
    const uint32_t* src;
    uint32_t* dst;
    long n4;
    int vec;
};

// this workgroup's chunk (blockIdx.x of gridDim.x, `nt` threads each) of row `srow` of src -> row `drow` of dst; a NULL pair is skipped
__device__ __forceinline__ void row_copy(const RowCopy& c, long srow, long drow, int nt) {
    if (!c.src) return;   // (uniform)
    const long i0 = (long)blockIdx.x * nt + threadIdx.x, step = (long)gridDim.x * nt;
    if (c.vec) {
        const uint4* const s = reinterpret_cast<const uint4*>(c.src + srow * c.n4);
        uint4* const d = reinterpret_cast<uint4*>(c.dst + drow * c.n4);
        for (long i = i0; i < c.n4 / 4; i += step) d[i] = s[i];
    } else {
        const uint32_t* const s = c.src + srow * c.n4;
        uint32_t* const d = c.dst + drow * c.n4;
        for (long i = i0; i < c.n4; i += step) d[i] = s[i];
    }
}

inline RowCopy make_row_copy(const void* src, void* dst, long n4) {
    RowCopy c;
    c.src = static_cast<const uint32_t*>(src);
    c.dst = static_cast<uint32_t*>(dst);
    c.n4 = n4;
    c.vec = src && (n4 % 4 == 0) && (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
    return c;
}
