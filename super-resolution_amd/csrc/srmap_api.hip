// srmap_api.hip -- what the C ABI (include/srmap.h) of the MI355X MAP gradient path has besides its jobs: the error text,
// the version string and the context.  The jobs: problem.hip (set-up and the model's setters), transfer.hip (host <->
// device copies), eval.hip (one evaluation, the operators on host buffers), data_weights.hip (the robust data term),
// solver.hip (the solves).
#include <cstdarg>
#include <new>

#include "srmap_internal.hpp"

using namespace srmap;

namespace srmap {

int set_error(srmap_ctx* ctx, int status, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (ctx) ctx->error = buf;
  return status;
}

}  // namespace srmap

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" {

const char* srmap_version(void) { return "srmap 0.1 (HIP, gfx950)"; }

long long srmap_live_allocations(void) { return g_live_allocations.load(); }

int srmap_ctx_create(int device_id, srmap_ctx** out) {
  if (!out) return SRMAP_EINVAL;
  *out = nullptr;
  srmap_ctx* ctx = new (std::nothrow) srmap_ctx();
  if (!ctx) return SRMAP_ENOMEM;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0 || device_id < 0 || device_id >= ndev) {
    fprintf(stderr, "srmap: no usable HIP device %d (%s); this library has no CPU path\n",
            device_id, e != hipSuccess ? hipGetErrorString(e) : "device index out of range");
    delete ctx;
    return SRMAP_EHIP;
  }
  ctx->device = device_id;
  if (hipSetDevice(device_id) != hipSuccess || hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
    delete ctx;
    return SRMAP_EHIP;
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) ctx->num_cus = prop.multiProcessorCount;
  *out = ctx;
  return SRMAP_OK;
}

void srmap_ctx_destroy(srmap_ctx* ctx) {
  if (!ctx) return;
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  for (int i = 0; i < 2; ++i)
    if (ctx->h_event[i]) (void)hipEventDestroy(ctx->h_event[i]);
  blas_release(ctx);
  delete ctx;  // and its pinned staging
}

const char* srmap_last_error(const srmap_ctx* ctx) { return ctx ? ctx->error.c_str() : "null context"; }

}  // extern "C"
