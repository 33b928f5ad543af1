// kbbq_lib_host.h -- what the host C++ files of libkbbq_hip.so share with the GPU half (internal: never installed, not part of
// the ABI).  No HIP types: every .cpp includes it; kbbq_lib.h adds what the .hip units share among themselves.
#pragma once
#include "../../include/kbbq_hip.h"

// the calling thread's error text, as kbbq_last_error returns it (kbbq_context.hip); returns `code`
int kbbq_set_error_(int code, const char* msg);

// for comm_rccl.cpp (kbbq_context.hip): the context's launch stream (a hipStream_t) and its device
extern "C" void* kbbq_ctx_stream_(kbbq_ctx* c);
extern "C" int kbbq_ctx_device_(kbbq_ctx* c);
