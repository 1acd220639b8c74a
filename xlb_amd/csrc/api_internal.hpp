// What the library's translation units share and the public header does not show: field helpers, the argument checks more than one
// stepper makes, the dispatchers on lattice and compute dtype, and the owners of device / pinned memory.
#pragma once
#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

#include "common.hpp"
#include "ops_kernels.hpp"

namespace xlb {

// new contents version of a field (api.hip owns the counter)
void touch(xlbhip_field* f);
// telemetry of the slab protocol: adds a completed halo wait of `slot` to the context's totals (api.hip)
int harvest_wait(xlbhip_ctx* c, int slot);

static FieldView view(const xlbhip_field* f) {
  FieldView v;
  v.data = f ? f->data : nullptr;
  v.plane_stride = f ? f->plane_stride : 0;
  v.dtype = f ? f->dtype : 0;
  v.halo = f ? f->halo : 0;
  return v;
}
static Dims dims(const xlbhip_field* f) { return Dims{f->nx, f->ny, f->nz}; }
static bool same_grid(const xlbhip_field* a, const xlbhip_field* b) { return a->nx == b->nx && a->ny == b->ny && a->nz == b->nz; }
static bool is_float(int dt) { return dt == XLBHIP_F64 || dt == XLBHIP_F32 || dt == XLBHIP_F16; }
static unsigned blocks_for(size_t n, int threads = 256) { return (unsigned)((n + threads - 1) / threads); }
// for the grid-stride kernels (k_copy, k_fill): HIP refuses launches of 2^32 threads or more
static unsigned blocks_capped(size_t n, int threads = 256) { return (unsigned)std::min<size_t>((n + threads - 1) / threads, (size_t)1 << 23); }

#define XLB_CHECK_POP(f, lattice, what)                                                                     \
  XLB_REQUIRE((f) && is_float((f)->dtype) && (f)->card == lattice_q(lattice), "%s: expected a %d-population float field", \
              what, lattice_q(lattice))

// a relaxation rate, `name` as the caller's argument is called
static int check_relaxation(const char* name, double omega) {
  XLB_REQUIRE(std::isfinite(omega) && omega > 0.0 && omega <= 2.0, "%s %g outside (0, 2]", name, omega);
  return 0;
}

// What the single-rank steppers (scalar transport, adjoint) ask of the grid `g` of their fields and of the two masks: an x plane the
// row kernels can address, a 2-D grid as one x plane, and with boundary conditions both masks on that grid without ghost planes.
// `who` / `kernel`: how the caller's plane-size message names itself and its kernel.
static int check_single_rank_grid(const char* who, const char* kernel, int lattice, int n_bc, const xlbhip_field* g, const xlbhip_field* bcm,
                                  const xlbhip_field* miss) {
  // the kernel's per-thread offsets inside an x plane are 32-bit byte offsets (8-byte elements, 4-byte missing words)
  XLB_REQUIRE((size_t)g->ny * g->nz <= ((size_t)1 << 28), "%s: an x plane of %d x %d cells is too large for the %s", who, g->ny, g->nz, kernel);
  XLB_REQUIRE(lattice != XLBHIP_D2Q9 || g->nx == 1, "a 2-D grid is stored as one x plane (%d given)", g->nx);
  if (n_bc > 0) {
    XLB_REQUIRE(bcm && bcm->dtype == XLBHIP_U8 && bcm->card == 1 && same_grid(bcm, g) && bcm->halo == 0, "bad or missing bc_mask field");
    XLB_REQUIRE(miss && miss->dtype == XLBHIP_MISSING && same_grid(miss, g) && miss->halo == 0, "bad or missing missing_mask field");
  }
  return 0;
}

template <class F>
static int by_lattice(int lattice, F&& f) {
  switch (lattice) {
    case XLBHIP_D2Q9: return f(D2Q9{});
    case XLBHIP_D3Q19: return f(D3Q19{});
    case XLBHIP_D3Q27: return f(D3Q27{});
  }
  XLB_FAIL("unknown lattice id %d", lattice);
}

// f(T{}) with T the compute dtype `cdt` (XLBHIP_F32 or XLBHIP_F64, checked by the caller)
template <class F>
static int by_compute(int cdt, F&& f) {
  return cdt == XLBHIP_F32 ? f(float{}) : f(double{});
}

// Move-only owner of one allocation: hipMalloc / hipFree, or hipHostMalloc / hipHostFree for PINNED host memory.  hipFree
// synchronises with the device, and callers rely on it: a buffer may be released while launches that read it are still queued.
template <bool PINNED>
class Buffer {
  void* p_ = nullptr;

 public:
  Buffer() = default;
  Buffer(Buffer&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
  Buffer& operator=(Buffer&& o) noexcept {
    if (this != &o) {
      (void)reset();
      p_ = std::exchange(o.p_, nullptr);
    }
    return *this;
  }
  Buffer(const Buffer&) = delete;
  Buffer& operator=(const Buffer&) = delete;
  ~Buffer() { (void)reset(); }
  // releases what it holds first; holds nothing after a failure
  hipError_t alloc(size_t bytes) {
    if (hipError_t e = reset(); e != hipSuccess) return e;
    const hipError_t e = PINNED ? hipHostMalloc(&p_, bytes, hipHostMallocDefault) : hipMalloc(&p_, bytes);
    if (e != hipSuccess) p_ = nullptr;
    return e;
  }
  hipError_t reset() {
    void* p = std::exchange(p_, nullptr);
    if (!p) return hipSuccess;
    return PINNED ? hipHostFree(p) : hipFree(p);
  }
  template <class T = void>
  T* get() const {
    return static_cast<T*>(p_);
  }
  explicit operator bool() const { return p_ != nullptr; }
};
using DeviceBuf = Buffer<false>;
using PinnedBuf = Buffer<true>;

// Device temporaries of one call on stream `st`: released on every exit path, after the stream has drained (copies and kernels
// may still use them).
struct DeviceScratch {
  hipStream_t st;
  std::vector<DeviceBuf> bufs;
  explicit DeviceScratch(hipStream_t s) : st(s) {}
  ~DeviceScratch() { (void)hipStreamSynchronize(st); }  // (the members go after this body)
  template <class P>
  hipError_t alloc(P** out, size_t bytes) {
    DeviceBuf b;
    const hipError_t e = b.alloc(bytes);
    *out = b.get<P>();
    if (e == hipSuccess) bufs.push_back(std::move(b));
    return e;
  }
};

// the 27 values of a BC descriptor in the compute dtype
template <class T>
static BcValues<T> bc_values(const double* v) {
  BcValues<T> out;
  for (int l = 0; l < 27; ++l) out.v[l] = static_cast<T>(v[l]);
  return out;
}

// `v` as host bytes in the compute dtype
static std::vector<char> compute_image(int cdt, const std::vector<double>& v) {
  std::vector<char> image;
  by_compute(cdt, [&](auto T) {
    const std::vector<decltype(T)> w(v.begin(), v.end());
    image.assign(reinterpret_cast<const char*>(w.data()), reinterpret_cast<const char*>(w.data() + w.size()));
    return 0;
  });
  return image;
}

// blocking upload of a host array into `out` (re-allocated; released and left empty for an empty array)
static int upload_bytes(const void* host, size_t bytes, DeviceBuf& out) {
  if (bytes == 0) {
    XLB_HIP(out.reset());
    return 0;
  }
  XLB_HIP(out.alloc(bytes));
  XLB_HIP(hipMemcpy(out.get(), host, bytes, hipMemcpyHostToDevice));
  return 0;
}
// a table of values, converted to the compute dtype
static int upload_values(int cdt, const std::vector<double>& v, DeviceBuf& out) {
  const std::vector<char> image = compute_image(cdt, v);
  return upload_bytes(image.data(), image.size(), out);
}
// the sorted storage-cell keys of a table
static int upload_keys(const std::vector<uint32_t>& keys, DeviceBuf& out) { return upload_bytes(keys.data(), keys.size() * sizeof(uint32_t), out); }

}  // namespace xlb
