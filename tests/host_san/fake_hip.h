// fake_hip.h -- what a sanitizer driver (drive_*.cpp, through drive_common.h) calls in the stand-in HIP runtime: the probes of
// fake_hip.cpp and the few hip* functions a driver calls itself.  fake_hip.cpp includes this header too, so a definition whose
// signature drifts from a declaration here does not compile (the functions have C linkage: no overloads).
#pragma once
#include <cstddef>

extern "C" {
typedef int hipError_t;
typedef struct fake_stream *hipStream_t;

long long fake_hip_launches(void);                           // kernel launches so far
long long fake_hip_copies(void);                             // hipMemcpy + hipMemcpyAsync calls so far
unsigned long long fake_hip_trace_hash(void);                // FNV-1a over the launch lines
unsigned long long fake_hip_copy_hash(int restart);          // ... over the copy / memset lines; restart: begin a new hash after this call
void fake_hip_trace_flush(void);                             // the FAKE_HIP_TRACE file is complete up to here
void fake_hip_fail_malloc_after(long long n);                // n more hipMalloc calls succeed, the next one fails; n < 0: off

hipError_t hipMalloc(void **p, size_t n);
hipError_t hipFree(void *p);
hipError_t hipMemsetAsync(void *d, int v, size_t n, hipStream_t s);   // a line "memset <bytes>" in the trace
}
