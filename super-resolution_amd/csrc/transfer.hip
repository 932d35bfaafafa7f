// transfer.hip -- host <-> device transfers of caller buffers: the pinned staging, the conversions between the caller's
// doubles and the problem dtype, and the C entry points that are nothing else.
#include <cstring>

#include "srmap_internal.hpp"

using namespace srmap;

namespace srmap {

template <typename T>
__global__ void k_from_double(const double* __restrict__ src, T* __restrict__ dst, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = (T)src[i];
}
template <typename T>
__global__ void k_to_double(const T* __restrict__ src, double* __restrict__ dst, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = (double)src[i];
}

// Caller buffers are pageable.  A plain hipMemcpy of them runs at 2-6 GB/s; two
// pinned chunks pipeline the PCIe transfer against the host-side memcpy.
constexpr size_t kStageBytes = 4u << 20;

int ensure_staging(srmap_ctx* ctx) {
  for (int i = 0; i < 2; ++i) {
    if (!ctx->h_stage[i]) SRMAP_HIP(ctx, ctx->h_stage[i].alloc(kStageBytes, hipHostMallocDefault));
    if (!ctx->h_event[i]) SRMAP_HIP(ctx, hipEventCreateWithFlags(&ctx->h_event[i], hipEventDisableTiming));
  }
  if (!ctx->h_scal) {
    SRMAP_HIP(ctx, ctx->h_scal.alloc(kHsSlots * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent));
    for (int i = 0; i < kHsSlots; ++i) ctx->h_scal.as<double>()[i] = 0.0;
  }
  return SRMAP_OK;
}

static int staged_h2d(srmap_ctx* ctx, void* dev, const void* host, size_t bytes, hipStream_t st) {
  int rc = ensure_staging(ctx);
  if (rc) return rc;
  size_t off = 0;
  for (int i = 0; off < bytes; ++i, off += kStageBytes) {
    const size_t nb = bytes - off < kStageBytes ? bytes - off : kStageBytes;
    const int b = i & 1;
    if (i >= 2) SRMAP_HIP(ctx, hipEventSynchronize(ctx->h_event[b]));  // chunk i-2 has left the buffer
    std::memcpy(ctx->h_stage[b].as(), (const char*)host + off, nb);
    SRMAP_HIP(ctx, hipMemcpyAsync((char*)dev + off, ctx->h_stage[b].as(), nb, hipMemcpyHostToDevice, st));
    SRMAP_HIP(ctx, hipEventRecord(ctx->h_event[b], st));
  }
  SRMAP_HIP(ctx, hipStreamSynchronize(st));
  return SRMAP_OK;
}

static int staged_d2h(srmap_ctx* ctx, void* host, const void* dev, size_t bytes, hipStream_t st) {
  int rc = ensure_staging(ctx);
  if (rc) return rc;
  const size_t nchunks = (bytes + kStageBytes - 1) / kStageBytes;
  for (size_t i = 0; i <= nchunks; ++i) {
    if (i < nchunks) {  // chunk i -> pinned buffer (its previous content, chunk i-2, was copied out below)
      const size_t off = i * kStageBytes, nb = bytes - off < kStageBytes ? bytes - off : kStageBytes;
      SRMAP_HIP(ctx, hipMemcpyAsync(ctx->h_stage[i & 1].as(), (const char*)dev + off, nb, hipMemcpyDeviceToHost, st));
      SRMAP_HIP(ctx, hipEventRecord(ctx->h_event[i & 1], st));
    }
    if (i >= 1) {  // chunk i-1 -> caller, while chunk i is on the wire
      const size_t off = (i - 1) * kStageBytes, nb = bytes - off < kStageBytes ? bytes - off : kStageBytes;
      SRMAP_HIP(ctx, hipEventSynchronize(ctx->h_event[(i - 1) & 1]));
      std::memcpy((char*)host + off, ctx->h_stage[(i - 1) & 1].as(), nb);
    }
  }
  return SRMAP_OK;
}

int convert_upload(srmap_problem* p, const double* host, void* dev, size_t n, hipStream_t st) {
  if (p->dtype == SRMAP_F64) return staged_h2d(p->ctx, dev, host, n * 8, st);
  DevBuf tmp;  // read by the conversion kernel: the stream is waited for before it goes
  SRMAP_HIP(p->ctx, tmp.alloc(n * 8));
  if (int rc = staged_h2d(p->ctx, tmp.as(), host, n * 8, st)) return rc;
  hipLaunchKernelGGL(k_from_double<float>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                     tmp.as<const double>(), (float*)dev, n);
  SRMAP_HIP(p->ctx, hipStreamSynchronize(st));
  return SRMAP_OK;
}

int convert_download(srmap_problem* p, const void* dev, double* host, size_t n, hipStream_t st) {
  if (p->dtype == SRMAP_F64) return staged_d2h(p->ctx, host, dev, n * 8, st);
  DevBuf tmp;
  SRMAP_HIP(p->ctx, tmp.alloc(n * 8));
  hipLaunchKernelGGL(k_to_double<float>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                     (const float*)dev, tmp.as<double>(), n);
  return staged_d2h(p->ctx, host, tmp.as(), n * 8, st);
}

int stage_host_x(srmap_problem* p, const double* x_host) {
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  const size_t n = p->hr_count();
  if (int rc = ensure(p, &p->d_x, n * p->elem())) return rc;
  return convert_upload(p, x_host, p->d_x.as(), n, p->ctx->stream);
}

}  // namespace srmap

extern "C" {

int srmap_device_alloc(srmap_ctx* ctx, size_t bytes, void** dev) {
  if (!ctx || !dev) return SRMAP_EINVAL;
  SRMAP_HIP(ctx, hipSetDevice(ctx->device));
  DevBuf b;  // handed to the caller, who returns it through srmap_device_free
  SRMAP_HIP(ctx, b.alloc(bytes));
  *dev = b.release();
  return SRMAP_OK;
}
int srmap_device_free(srmap_ctx* ctx, void* dev) {
  if (!ctx) return SRMAP_EINVAL;
  if (dev) SRMAP_HIP(ctx, hipFree(dev));
  return SRMAP_OK;
}
int srmap_upload(srmap_problem* p, const double* host, void* dev, size_t count) {
  if (!p || !host || !dev) return SRMAP_EINVAL;
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  return convert_upload(p, host, dev, count, p->ctx->stream);
}
int srmap_download(srmap_problem* p, const void* dev, double* host, size_t count) {
  if (!p || !host || !dev) return SRMAP_EINVAL;
  SRMAP_HIP(p->ctx, hipSetDevice(p->ctx->device));
  return convert_download(p, dev, host, count, p->ctx->stream);
}
int srmap_synchronize(srmap_ctx* ctx) {
  if (!ctx) return SRMAP_EINVAL;
  SRMAP_HIP(ctx, hipSetDevice(ctx->device));
  SRMAP_HIP(ctx, hipDeviceSynchronize());
  return SRMAP_OK;
}

}  // extern "C"
