// starch_amd/csrc/api_core.hip -- the C ABI (include/starch_amd.h): version and errors,
// contexts and their streams, default options, host registration, and the
// result of the decode, sort, bedops and bedmap calls (starch_output_*).
#include <string.h>

#include <chrono>
#include <mutex>

#include "api_int.hpp"

namespace api {

// STARCH_TRACE=1: host-side timeline of the batched paths on stderr
double trace_t0()
{
    static const auto t0 = std::chrono::steady_clock::now();
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
bool tracing()
{
    static const bool on = getenv("STARCH_TRACE") != nullptr;
    return on;
}

}  // namespace api

using namespace api;

extern "C" {

int starch_version(void) { return 0x000100; }

const char* starch_strerror(int code)
{
    switch (code) {
        case STARCH_OK: return "ok";
        case STARCH_ERR_ARG: return "invalid argument";
        case STARCH_ERR_MEM: return "out of memory or buffer too small";
        case STARCH_ERR_STATE: return "no result available";
        case STARCH_ERR_DEVICE: return "HIP device error";
        case STARCH_ERR_DATA: return "malformed or corrupt compressed data";
        default: return "internal error";
    }
}

const char* starch_last_error(starch_ctx* ctx) { return ctx ? ctx->err.c_str() : "no context"; }

int starch_create(int device, starch_ctx** out)
{
    if (!out) return STARCH_ERR_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return STARCH_ERR_DEVICE;
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, device) != hipSuccess) return STARCH_ERR_DEVICE;
    if (strncmp(p.gcnArchName, "gfx950", 6) != 0) return STARCH_ERR_DEVICE;   // code objects are gfx950-only
    starch_ctx* c = new starch_ctx();
    c->device = device;
    int prev = 0;
    (void)hipGetDevice(&prev);
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return STARCH_ERR_DEVICE;
    }
    (void)hipSetDevice(prev);
    c->st = c->own;
    *out = c;
    return STARCH_OK;
}

void starch_destroy(starch_ctx* c)
{
    if (!c) return;
    c->stream_shutdown();
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->st);
    if (c->cst) (void)hipStreamDestroy(c->cst);
    if (c->own) (void)hipStreamDestroy(c->own);
    delete c;
}

int starch_set_stream(starch_ctx* c, void* s)
{
    if (!c) return STARCH_ERR_ARG;
    c->st = static_cast<hipStream_t>(s);   // NULL = the HIP null stream (include/starch_amd.h)
    return STARCH_OK;
}

int starch_set_lanes(starch_ctx* c, int lanes)
{
    if (!c || lanes < 0 || lanes > 8) return STARCH_ERR_ARG;
    GUARD(c)
    c->dev_lanes = lanes;
    if (lanes == 1)   // the extra lanes' encoders give their HBM back (one encoder now holds every block)
        for (auto& l : c->lanes) {
            HIP_CHECK(hipStreamSynchronize(l->st));
            l->enc.release_device();
        }
    return STARCH_OK;
    END_GUARD(c)
}

int starch_use_own_stream(starch_ctx* c)
{
    if (!c) return STARCH_ERR_ARG;
    c->st = c->own;
    return STARCH_OK;
}

void starch_options_init(starch_options* o)
{
    if (!o) return;
    o->block_size_100k = 9;
    o->emit_index = 1;
    o->reference_compat = 0;
    o->note = nullptr;
    o->base_counts = 0;
    o->compression_method = STARCH_METHOD_BZIP2;
}

int starch_host_register(const void* p, uint64_t n)
{
    const uintptr_t pg = 4096, b = reinterpret_cast<uintptr_t>(p);
    const uintptr_t l = (b + pg - 1) & ~(pg - 1), h = (b + n) & ~(pg - 1);
    if (!p || h <= l) return STARCH_ERR_ARG;
    PinRegistry& R = pin_registry();
    std::lock_guard<std::mutex> lk(R.mu);
    if (R.overlaps(l, h)) return STARCH_ERR_ARG;            // (already registered, or in use by a call)
    bool ok = hipHostRegister(reinterpret_cast<void*>(l), h - l, hipHostRegisterPortable) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();   // a read-only mapping (a mapped input file): registered for reads
        ok = hipHostRegister(reinterpret_cast<void*>(l), h - l, hipHostRegisterReadOnly | hipHostRegisterPortable) == hipSuccess;
    }
    if (!ok) {
        (void)hipGetLastError();
        return STARCH_ERR_DEVICE;
    }
    R.m[l] = PinRegistry::Range{h, 0, false};               // the library DMAs from [l, h) only
    return STARCH_OK;
}

int starch_host_unregister(const void* p)
{
    const uintptr_t pg = 4096, l = (reinterpret_cast<uintptr_t>(p) + pg - 1) & ~(pg - 1);
    if (!p) return STARCH_ERR_ARG;
    PinRegistry& R = pin_registry();
    std::lock_guard<std::mutex> lk(R.mu);
    auto it = R.m.find(l);
    if (it == R.m.end() || it->second.temp) return STARCH_ERR_ARG;
    R.m.erase(it);
    if (hipHostUnregister(reinterpret_cast<void*>(l)) != hipSuccess) {
        (void)hipGetLastError();
        return STARCH_ERR_DEVICE;
    }
    return STARCH_OK;
}

int starch_output_size(starch_ctx* c, uint64_t* n)
{
    if (!c || !n) return STARCH_ERR_ARG;
    if (!c->have_out) return STARCH_ERR_STATE;
    *n = c->out_bytes;
    return STARCH_OK;
}

int starch_output_device(starch_ctx* c, const void** d_ptr)
{
    if (!c || !d_ptr) return STARCH_ERR_ARG;
    if (!c->have_out) return STARCH_ERR_STATE;
    *d_ptr = c->out_dev;
    return STARCH_OK;
}

int starch_output_copy(starch_ctx* c, void* dst, uint64_t cap)
{
    GUARD(c)
    if (!c->have_out) return STARCH_ERR_STATE;
    if (cap < c->out_bytes || (c->out_bytes && !dst)) return STARCH_ERR_MEM;
    if (c->out_bytes) HIP_CHECK(hipMemcpyAsync(dst, c->out_dev, c->out_bytes, hipMemcpyDeviceToHost, c->st));
    HIP_CHECK(hipStreamSynchronize(c->st));
    return STARCH_OK;
    END_GUARD(c)
}

}  // extern "C"
