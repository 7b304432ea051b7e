// fake_hip.cpp -- a FUNCTIONAL stand-in for the HIP runtime, for the sanitizer builds of liblpf's HOST side only
// (tests/host_san/Makefile; never part of the product, never used on a GPU box).  lpf_api.hip is compiled with
// `hipcc --offload-host-only -fsanitize=...` and linked against this file instead of libamdhip64: device memory is host memory
// (calloc), copies are memcpy at the time of the call, kernel launches do nothing, streams / events / graphs are bookkeeping
// objects.  What runs under ASan / UBSan / TSan is therefore everything the host code does around the launches: argument
// validation, the pinned upload ring, the rotation of scratch sets and box sets, the table builders, the graph state machine and
// the reader's worker threads -- with every "device" and "pinned" buffer a heap block whose bounds the sanitizer knows.
// Which kernels the host code launches, and with which grids, is recorded: every launch is a line "<kernel> gx gy gz bx by bz" (the
// kernel's mangled name as the code object lists it; no pointer-valued arguments -- they differ from run to run), folded into a running
// hash (fake_hip_trace_hash) and written to the file FAKE_HIP_TRACE names, if it is set.  Two builds of the host code that launch the
// same kernels in the same order have the same hash and the same launch lines.  Copies and memsets are recorded beside them, as
// "copy <kind> <bytes>" (hipMemcpyKind's number: 1 up, 2 down, 3 device to device) and "memset <bytes>" -- no pointers either -- in the
// same file, where they stand between the launches they were queued between, and folded into a hash of their own
// (fake_hip_copy_hash, which a driver may restart per section: threads that copy, the reader's workers, make the order of one
// section's lines differ from run to run), so that the launch hash means what it always did.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <map>
#include <mutex>
#include <string>

#include "fake_hip.h"

extern "C" {

struct fake_stream { int capturing; };
typedef struct fake_event { std::atomic<int> recorded; } *hipEvent_t;
typedef struct fake_graph { int n; } *hipGraph_t;
typedef struct fake_exec { int n; } *hipGraphExec_t;
struct dim3_ { unsigned x, y, z; };

static std::atomic<long long> g_launches{0}, g_copies{0};
long long fake_hip_launches(void) { return g_launches.load(); }
long long fake_hip_copies(void) { return g_copies.load(); }

// The launch trace.  Its state is a function-local static: hipcc's registration constructors (__hipRegisterFunction) run before this
// file's own static objects would be constructed.
namespace {
struct Trace {
    std::mutex mu;
    std::map<const void *, std::string> names;            // host stub -> kernel name
    unsigned long long hash = 1469598103934665603ull;     // FNV-1a over the launch lines ...
    unsigned long long copy_hash = 1469598103934665603ull;    // ... and over the copy / memset lines
    FILE *file = nullptr;
    bool opened = false;
};
Trace &trace() { static Trace *t = new Trace; return *t; }
void trace_line(const char *line, int n, unsigned long long Trace::*hash)
{
    Trace &t = trace();
    std::lock_guard<std::mutex> lock(t.mu);
    for (int i = 0; i < n; ++i) t.*hash = (t.*hash ^ (unsigned char)line[i]) * 1099511628211ull;
    if (!t.opened) {
        t.opened = true;
        const char *path = getenv("FAKE_HIP_TRACE");
        if (path && *path) t.file = fopen(path, "w");
    }
    if (t.file) fputs(line, t.file);
}
void trace_launch(const char *name, dim3_ g, dim3_ b)
{
    char line[640];
    const int n = snprintf(line, sizeof line, "%s %u %u %u %u %u %u\n", name, g.x, g.y, g.z, b.x, b.y, b.z);
    trace_line(line, n < (int)sizeof line ? n : (int)sizeof line - 1, &Trace::hash);
}
void trace_copy(int kind, size_t bytes)                   // kind < 0: a memset
{
    char line[64];
    const int n = kind < 0 ? snprintf(line, sizeof line, "memset %zu\n", bytes) : snprintf(line, sizeof line, "copy %d %zu\n", kind, bytes);
    trace_line(line, n, &Trace::copy_hash);
}
}  // namespace
unsigned long long fake_hip_trace_hash(void) { Trace &t = trace(); std::lock_guard<std::mutex> lock(t.mu); return t.hash; }
unsigned long long fake_hip_copy_hash(int restart)        // restart: the next call's hash covers what is copied from here on
{
    Trace &t = trace();
    std::lock_guard<std::mutex> lock(t.mu);
    const unsigned long long h = t.copy_hash;
    if (restart) t.copy_hash = 1469598103934665603ull;
    return h;
}
void fake_hip_trace_flush(void) { Trace &t = trace(); std::lock_guard<std::mutex> lock(t.mu); if (t.file) fflush(t.file); }

hipError_t hipGetDeviceCount(int *n) { *n = 1; return 0; }
hipError_t hipSetDevice(int) { return 0; }
hipError_t hipGetLastError(void) { return 0; }
const char *hipGetErrorString(hipError_t) { return "fake HIP error"; }

// A failing allocation, for a driver's error paths: after fake_hip_fail_malloc_after(n), n more hipMalloc calls succeed and the next ONE
// fails (hipErrorOutOfMemory); n < 0 disarms.  Off unless a driver arms it.
static std::atomic<long long> g_fail_malloc{-1};
void fake_hip_fail_malloc_after(long long n) { g_fail_malloc = n; }
hipError_t hipMalloc(void **p, size_t n)
{
    if (g_fail_malloc >= 0 && g_fail_malloc-- == 0) { *p = nullptr; return 2; }
    *p = calloc(n ? n : 1, 1);
    return *p ? 0 : 2;
}
hipError_t hipFree(void *p) { free(p); return 0; }
hipError_t hipHostMalloc(void **p, size_t n, unsigned) { *p = malloc(n ? n : 1); return *p ? 0 : 2; }
hipError_t hipHostFree(void *p) { free(p); return 0; }
hipError_t hipPointerGetAttributes(void *, const void *) { return 1; }      // (nothing is GPU-mapped here: host results take the copy path)
hipError_t hipMemcpy(void *d, const void *s, size_t n, int kind) { ++g_copies; trace_copy(kind, n); memmove(d, s, n); return 0; }
hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, int kind, hipStream_t) { ++g_copies; trace_copy(kind, n); memmove(d, s, n); return 0; }
hipError_t hipMemsetAsync(void *d, int v, size_t n, hipStream_t) { trace_copy(-1, n); memset(d, v, n); return 0; }

hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { *s = new fake_stream{0}; return 0; }
hipError_t hipStreamDestroy(hipStream_t s) { delete s; return 0; }
hipError_t hipStreamSynchronize(hipStream_t) { return 0; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { return 0; }
hipError_t hipStreamBeginCapture(hipStream_t s, int) { if (s) s->capturing = 1; return 0; }
hipError_t hipStreamEndCapture(hipStream_t s, hipGraph_t *g) { if (s) s->capturing = 0; *g = new fake_graph{1}; return 0; }

hipError_t hipEventCreate(hipEvent_t *e) { *e = new fake_event; (*e)->recorded = 0; return 0; }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return hipEventCreate(e); }
hipError_t hipEventDestroy(hipEvent_t e) { delete e; return 0; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t) { e->recorded = 1; return 0; }
hipError_t hipEventQuery(hipEvent_t) { return 0; }
hipError_t hipEventSynchronize(hipEvent_t) { return 0; }
hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) { *ms = 0.001f; return 0; }

hipError_t hipGraphInstantiate(hipGraphExec_t *x, hipGraph_t, void *, void *, size_t) { *x = new fake_exec{1}; return 0; }
hipError_t hipGraphLaunch(hipGraphExec_t, hipStream_t) { ++g_launches; trace_launch("hipGraphLaunch", dim3_{0, 0, 0}, dim3_{0, 0, 0}); return 0; }
hipError_t hipGraphDestroy(hipGraph_t g) { delete g; return 0; }
hipError_t hipGraphExecDestroy(hipGraphExec_t x) { delete x; return 0; }

// kernel launches: the host stubs hipcc generates push a launch configuration, pop it again and call hipLaunchKernel
static thread_local struct { dim3_ g, b; size_t shm; hipStream_t s; } t_cfg;
hipError_t __hipPushCallConfiguration(dim3_ g, dim3_ b, size_t shm, hipStream_t s) { t_cfg.g = g; t_cfg.b = b; t_cfg.shm = shm; t_cfg.s = s; return 0; }
hipError_t __hipPopCallConfiguration(dim3_ *g, dim3_ *b, size_t *shm, hipStream_t *s) { *g = t_cfg.g; *b = t_cfg.b; *shm = t_cfg.shm; *s = t_cfg.s; return 0; }
hipError_t hipLaunchKernel(const void *fn, dim3_ g, dim3_ b, void **, size_t, hipStream_t)
{
    if (g.x == 0 || b.x == 0 || b.x > 1024) { fprintf(stderr, "fake_hip: launch with grid %u block %u\n", g.x, b.x); abort(); }
    ++g_launches;
    const char *name = "?";
    {
        Trace &t = trace();
        std::lock_guard<std::mutex> lock(t.mu);
        auto it = t.names.find(fn);
        if (it != t.names.end()) name = it->second.c_str();     // (entries are never removed: the pointer stays good)
    }
    trace_launch(name, g, b);
    return 0;
}
void **__hipRegisterFatBinary(const void *) { static void *h; return &h; }
void __hipRegisterFunction(void **, const void *host_fn, char *, const char *device_name, unsigned, void *, void *, void *, void *, int *)
{
    Trace &t = trace();
    std::lock_guard<std::mutex> lock(t.mu);
    t.names[host_fn] = device_name;
}
void __hipRegisterVar(void **, void *, char *, const char *, int, size_t, int, int) {}
void __hipUnregisterFatBinary(void **) {}

}  // extern "C"
