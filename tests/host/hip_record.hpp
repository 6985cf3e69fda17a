// Recording stand-ins for the HIP runtime entry points the library calls: the two CPU recorders (launch_record.hip, enqueue_record.hip)
// link the library's objects against these instead of a runtime.  No GPU is opened, no kernel runs, "device" memory is host memory
// that nobody touches.  A kernel launch is handed to on_launch(), which the including program defines; every other call that orders
// work on a stream prints its own line while g_rec_on is set (enqueue_record.hip sets it around one operator call).
#pragma once
#include <cxxabi.h>
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "gemm_ops.hpp"

static void on_launch(const std::string& name, dim3 grid, dim3 block, size_t lds, hipStream_t st, void** args);

static std::map<const void*, std::string>& kernel_names() { static std::map<const void*, std::string> m; return m; }
static struct { dim3 grid, block; size_t lds; hipStream_t st; } g_cfg;

// ---- what the enqueue recorder names: streams and events in order of creation, allocations made inside a call -------------------------
static bool g_rec_on = false;
static std::map<const void*, std::string>& rec_names() { static std::map<const void*, std::string> m; return m; }
static std::map<const void*, size_t>& rec_allocs() { static std::map<const void*, size_t> m; return m; }   // made while g_rec_on
static int g_n_side = 0, g_n_ev = 0;
static const char* rec_name(const void* p) {
    if (!p) return "main";
    auto it = rec_names().find(p);
    return it == rec_names().end() ? "?" : it->second.c_str();
}
static void* rec_handle(const char* kind, int k) {   // a handle is a one-byte allocation: unique, non-null, never dereferenced
    void* h = malloc(1);
    rec_names()[h] = kind + std::to_string(k);
    return h;
}
static void rec_forget() {   // between engines: the next one numbers its side streams and events from 0 again
    for (auto& kv : rec_names()) free(const_cast<void*>(kv.first));
    rec_names().clear();
    g_n_side = g_n_ev = 0;
}

// "<name> grid=x,y,z wg=w lds=b" + the host-set switches of the GEMM operand structs
static void print_launch(const std::string& name, dim3 grid, dim3 block, size_t lds, void** args) {
    printf("%s grid=%u,%u,%u wg=%u lds=%zu", name.c_str(), grid.x, grid.y, grid.z, block.x, lds);
    if (name.compare(0, 13, "gemm3_kernel<") == 0) {
        const Gemm3Operands* g = static_cast<const Gemm3Operands*>(args[0]);
        printf(" nfast=%d stage16=%d", g->nfast, g->stage16);
    } else if (name.compare(0, 12, "gemm_kernel<") == 0) {
        printf(" xcd_order=%d", static_cast<const GemmOperands*>(args[0])->xcd_order);
    }
}

extern "C" {
void** __hipRegisterFatBinary(const void*) { static void* h; return &h; }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterVar(void**, void*, char*, char*, int, size_t, int, int) {}
void __hipRegisterFunction(void**, const void* host, char*, const char* device_name, unsigned, uint3*, uint3*, dim3*, dim3*, int*) {
    int status = 0;
    char* d = abi::__cxa_demangle(device_name, nullptr, nullptr, &status);
    std::string n = status == 0 && d ? d : device_name;
    free(d);
    if (n.compare(0, 5, "void ") == 0) n.erase(0, 5);
    for (size_t at; (at = n.find("(anonymous namespace)::")) != std::string::npos;) n.erase(at, 23);
    int depth = 0;   // cut the parameter list: the first '(' outside the template arguments
    for (size_t i = 0; i < n.size(); ++i) {
        if (n[i] == '<') ++depth;
        else if (n[i] == '>') --depth;
        else if (n[i] == '(' && depth == 0) { n.erase(i); break; }
    }
    std::string packed;
    for (char c : n)
        if (c != ' ') packed += c;
    kernel_names()[host] = packed;
}
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t lds, hipStream_t st) { g_cfg = {grid, block, lds, st}; return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* lds, hipStream_t* st) {
    *grid = g_cfg.grid; *block = g_cfg.block; *lds = g_cfg.lds; *st = g_cfg.st;
    return hipSuccess;
}
hipError_t hipLaunchKernel(const void* f, dim3 grid, dim3 block, void** args, size_t lds, hipStream_t st) {
    auto it = kernel_names().find(f);
    on_launch(it == kernel_names().end() ? "?" : it->second, grid, block, lds, st, args);
    return hipSuccess;
}
hipError_t hipFuncSetAttribute(const void*, hipFuncAttribute, int) { return hipSuccess; }
hipError_t hipGetDevice(int* dev) { *dev = 0; return hipSuccess; }
hipError_t hipGetDeviceCount(int* n) { *n = 1; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipDeviceGetAttribute(int* v, hipDeviceAttribute_t, int) { *v = 256; return hipSuccess; }
hipError_t hipGetLastError() { return hipSuccess; }
const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "error"; }
hipError_t hipDeviceSynchronize() { return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }

// memory: 256-byte aligned like the runtime's, never read or written by the library's host code
hipError_t hipMalloc(void** p, size_t bytes) {
    const size_t n = (bytes + 255) & ~size_t(255);
    *p = aligned_alloc(256, n ? n : 256);
    if (!*p) return hipErrorOutOfMemory;
    if (g_rec_on) rec_allocs()[*p] = bytes;
    return hipSuccess;
}
hipError_t hipFree(void* p) { rec_allocs().erase(p); free(p); return hipSuccess; }
// a memset over the whole of a buffer the call allocated itself (a test hook's private workspace) prints no size: how large a
// workspace is belongs to the layout, not to the enqueue sequence
static void rec_memset(const void* dst, size_t bytes, hipStream_t st) {
    if (!g_rec_on) return;
    auto it = rec_allocs().find(dst);
    if (it != rec_allocs().end() && it->second == bytes) printf("%s memset whole\n", rec_name(st));
    else printf("%s memset %zu\n", rec_name(st), bytes);
}
static void rec_memcpy(void* dst, size_t bytes, hipMemcpyKind kind, hipStream_t st) {
    static const char* const kinds[] = {"h2h", "h2d", "d2h", "d2d", "default"};
    if (kind == hipMemcpyDeviceToHost) memset(dst, 0, bytes);   // host code that reads weights back sees zeros
    if (g_rec_on) printf("%s memcpy %zu %s\n", rec_name(st), bytes, (unsigned)kind <= 4u ? kinds[kind] : "?");
}
hipError_t hipMemset(void* dst, int, size_t bytes) { rec_memset(dst, bytes, nullptr); return hipSuccess; }
hipError_t hipMemsetAsync(void* dst, int, size_t bytes, hipStream_t st) { rec_memset(dst, bytes, st); return hipSuccess; }
hipError_t hipMemcpy(void* dst, const void*, size_t bytes, hipMemcpyKind kind) { rec_memcpy(dst, bytes, kind, nullptr); return hipSuccess; }
hipError_t hipMemcpyAsync(void* dst, const void*, size_t bytes, hipMemcpyKind kind, hipStream_t st) { rec_memcpy(dst, bytes, kind, st); return hipSuccess; }
// (the codec's image copies, device to device only: rows of `width` bytes, `height` of them; the pitches belong to the layout)
hipError_t hipMemcpy2DAsync(void*, size_t, const void*, size_t, size_t width, size_t height, hipMemcpyKind kind, hipStream_t st) {
    if (kind != hipMemcpyDeviceToDevice) return hipErrorInvalidValue;
    if (g_rec_on) printf("%s memcpy2d %zux%zu d2d\n", rec_name(st), width, height);
    return hipSuccess;
}

// streams and events
hipError_t hipStreamCreateWithFlags(hipStream_t* st, unsigned) {
    *st = static_cast<hipStream_t>(rec_handle("side", g_n_side++));
    if (g_rec_on) printf("create %s\n", rec_name(*st));
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t) { return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* ev, unsigned) {
    *ev = static_cast<hipEvent_t>(rec_handle("ev", g_n_ev++));
    if (g_rec_on) printf("create %s\n", rec_name(*ev));
    return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t* ev) { return hipEventCreateWithFlags(ev, 0); }
hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t ev, hipStream_t st) {
    if (g_rec_on) printf("%s record %s\n", rec_name(st), rec_name(ev));
    return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t st, hipEvent_t ev, unsigned) {
    if (g_rec_on) printf("%s wait %s\n", rec_name(st), rec_name(ev));
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 0.f; return hipSuccess; }
}
