// CPU stand-in for the few HIP runtime entry points pyrad_amd/csrc/lbl_api.hip uses, for the sanitizer harness of the host
// shim (tests/host_shim/, tests/test_host_shim_asan_cpu.py).  TEST INFRASTRUCTURE: "device" memory is plain host memory (so that
// AddressSanitizer sees every copy the shim issues), streams and events are counters, graphs are empty.  Nothing here is ever
// linked into libpyrad_hip.so.
//
// Copies stay synchronous, but the ORDER the real runtime would give them is kept for page-locked sources: a host-to-device
// hipMemcpyAsync out of a live hipHostMalloc block gets a sequence number and its source range is poisoned
// (ASAN_POISON_MEMORY_REGION) until something the host waited for covers it - hipStreamSynchronize / hipDeviceSynchronize (every
// copy of that stream / of all), hipEventSynchronize(e) (the copies enqueued on e's stream before e was recorded), hipHostFree of
// the block.  A write into a range that a queued copy would still have to read is then an AddressSanitizer use-after-poison report.
#pragma once
#include <sanitizer/asan_interface.h>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>

typedef int hipError_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorInvalidValue = 1 };
struct mock_stream { int id; bool capturing; };
struct mock_event { long long stamp; long long copies; mock_stream* stream; };     // copies: the last staged copy enqueued before the record
struct mock_graph { int nodes; };
typedef mock_stream* hipStream_t;
typedef mock_event* hipEvent_t;
typedef mock_graph* hipGraph_t;
typedef mock_graph* hipGraphExec_t;
struct int2 { int x, y; };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2, hipMemcpyDeviceToDevice = 3, hipMemcpyDefault = 4 };
enum { hipStreamNonBlocking = 1, hipEventDisableTiming = 2, hipHostMallocDefault = 0 };
enum hipStreamCaptureMode { hipStreamCaptureModeGlobal = 0, hipStreamCaptureModeThreadLocal = 1 };
struct hipDeviceProp_t { char name[256]; int multiProcessorCount; size_t totalGlobalMem; char gcnArchName[256]; };

namespace mockhip {
extern int device_count;            // what hipGetDeviceCount reports (the driver sets it)
extern long long fail_malloc_at;    // the n-th hipMalloc from now fails with hipErrorOutOfMemory (-1: never)
extern long long clock;
extern long long live_allocs, live_streams, live_events, live_graphs, live_host;
extern long long launches;          // stand-in launchers entered so far (mock_kernels.cpp)
extern long long staged_copies;     // host-to-device hipMemcpyAsync calls out of a page-locked block so far (the sequence number of the last)
extern long long staged_on_middle;  // ... whose source, rounded up to the 256 bytes the shim allocates in, ended exactly on the middle of its block
extern long long staged_rewrites;   // ... whose source range had been copied out of before: the shim wrote it again in between
extern long long stream_syncs;      // hipStreamSynchronize + hipDeviceSynchronize calls so far
void host_block_made(void* p, size_t bytes);
void host_block_freed(void* p);                                        // retires what is pending in it
void staged_copy(const void* src, size_t n, mock_stream* stream);      // after the copy: counts it and poisons its source if page-locked
void before_read(const void* src, size_t n);                           // a copy may READ a range that is still pending ...
void after_read();                                                     // ... which stays pending
void retire(mock_stream* stream, long long up_to);                     // stream == nullptr: every stream
}

inline const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "success" : e == hipErrorOutOfMemory ? "out of memory (mock)" : "error (mock)"; }
inline hipError_t hipGetLastError() { return hipSuccess; }
inline hipError_t hipGetDeviceCount(int* n) { *n = mockhip::device_count; return hipSuccess; }
inline hipError_t hipSetDevice(int d) { return d >= 0 && d < mockhip::device_count ? hipSuccess : hipErrorInvalidValue; }
inline hipError_t hipGetDeviceProperties(hipDeviceProp_t* p, int) {
    memset(p, 0, sizeof *p); strcpy(p->name, "mock gfx950"); strcpy(p->gcnArchName, "gfx950"); p->multiProcessorCount = 256;
    p->totalGlobalMem = (size_t)288 << 30; return hipSuccess;
}
inline hipError_t hipMalloc(void** p, size_t bytes) {
    if (mockhip::fail_malloc_at >= 0 && mockhip::fail_malloc_at-- == 0) { *p = nullptr; return hipErrorOutOfMemory; }
    if (posix_memalign(p, 256, bytes ? bytes : 1)) { *p = nullptr; return hipErrorOutOfMemory; }     // hipMalloc returns 256-byte aligned blocks
    memset(*p, 0xA5, bytes);           // a read of "uninitialised device memory" is at least not zeros
    ++mockhip::live_allocs; return hipSuccess;
}
inline hipError_t hipFree(void* p) { if (p) { free(p); --mockhip::live_allocs; } return hipSuccess; }
inline hipError_t hipHostMalloc(void** p, size_t bytes, unsigned = 0) {
    *p = malloc(bytes ? bytes : 1); if (!*p) return hipErrorOutOfMemory;
    ++mockhip::live_host; mockhip::host_block_made(*p, bytes ? bytes : 1); return hipSuccess;
}
inline hipError_t hipHostFree(void* p) { if (p) { mockhip::host_block_freed(p); free(p); --mockhip::live_host; } return hipSuccess; }
inline hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind) { mockhip::before_read(s, n); memmove(d, s, n); mockhip::after_read(); return hipSuccess; }
inline hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind kind, hipStream_t stream) {
    mockhip::before_read(s, n);
    memmove(d, s, n);
    if (kind == hipMemcpyHostToDevice) mockhip::staged_copy(s, n, stream);
    mockhip::after_read();
    return hipSuccess;
}
inline hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t) { memset(d, v, n); return hipSuccess; }
inline hipError_t hipMemsetD32(void* d, int v, size_t count) { for (size_t i = 0; i < count; ++i) ((int*)d)[i] = v; return hipSuccess; }
inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { *s = new mock_stream{0, false}; ++mockhip::live_streams; return hipSuccess; }
inline hipError_t hipStreamDestroy(hipStream_t s) { delete s; --mockhip::live_streams; return hipSuccess; }
inline hipError_t hipStreamSynchronize(hipStream_t s) { ++mockhip::stream_syncs; mockhip::retire(s, mockhip::staged_copies); return hipSuccess; }
inline hipError_t hipDeviceSynchronize() { ++mockhip::stream_syncs; mockhip::retire(nullptr, mockhip::staged_copies); return hipSuccess; }
inline hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { return hipSuccess; }
inline hipError_t hipEventCreate(hipEvent_t* e) { *e = new mock_event{0, 0, nullptr}; ++mockhip::live_events; return hipSuccess; }
inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return hipEventCreate(e); }
inline hipError_t hipEventDestroy(hipEvent_t e) { delete e; --mockhip::live_events; return hipSuccess; }
inline hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { e->stamp = ++mockhip::clock; e->copies = mockhip::staged_copies; e->stream = s; return hipSuccess; }
inline hipError_t hipEventSynchronize(hipEvent_t e) {
    // (self-test of the harness, tests/test_host_shim_asan_cpu.py: with SHIM_INJECT_NO_EVENT_WAIT set waiting for an event covers
    // nothing, as if the shim had not waited: a page-locked block written again too early must then be reported)
    static const bool covers_nothing = getenv("SHIM_INJECT_NO_EVENT_WAIT") != nullptr;
    if (!covers_nothing && e->stream) mockhip::retire(e->stream, e->copies);
    return hipSuccess;
}
inline hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) { *ms = (float)(b->stamp - a->stamp) * 1e-3f; return hipSuccess; }
inline hipError_t hipStreamBeginCapture(hipStream_t s, hipStreamCaptureMode) { s->capturing = true; return hipSuccess; }
inline hipError_t hipStreamEndCapture(hipStream_t s, hipGraph_t* g) { s->capturing = false; *g = new mock_graph{1}; ++mockhip::live_graphs; return hipSuccess; }
inline hipError_t hipGraphInstantiate(hipGraphExec_t* x, hipGraph_t, void*, void*, size_t) { *x = new mock_graph{1}; ++mockhip::live_graphs; return hipSuccess; }
inline hipError_t hipGraphLaunch(hipGraphExec_t, hipStream_t) { return hipSuccess; }
inline hipError_t hipGraphDestroy(hipGraph_t g) { delete g; --mockhip::live_graphs; return hipSuccess; }
inline hipError_t hipGraphExecDestroy(hipGraphExec_t g) { delete g; --mockhip::live_graphs; return hipSuccess; }
