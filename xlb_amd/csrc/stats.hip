// libxlbhip: FlowStatistics (stats_kernels.hpp).  The object owns the running sums, the scratch of the partial sums and the
// watchdog's words; a sample only enqueues on the context's compute stream, xlbhip_stats_read is the one call that waits.
#include <cstddef>
#include <cstring>
#include <memory>
#include <vector>

#include "api_internal.hpp"
#include "stats_kernels.hpp"

using namespace xlb;

struct xlbhip_stats {
  xlbhip_ctx* ctx = nullptr;
  int lattice = 0, cdt = 0, order = 2;
  StatsPlan plan{};
  StatsExclude exclude{};
  int channels = 0;
  int64_t samples = 0;
  DeviceBuf sums;     // double [channels][bins]
  DeviceBuf scratch;  // double [nj][channels][bins], only with nj > 1
  DeviceBuf watch;    // StatsWatch
  size_t cols() const { return (size_t)channels * (size_t)plan.bins; }
};

namespace xlb {

// fn(L{}, T{}, S{}, order) for the object's lattice and compute dtype and the field's store dtype
template <class Fn>
static int stats_dispatch(const xlbhip_stats* s, int sdt, Fn&& fn) {
  auto by_order = [&](auto L, auto T, auto S) {
    if (s->order == 2) return fn(L, T, S, std::integral_constant<int, 2>{});
    return fn(L, T, S, std::integral_constant<int, 1>{});
  };
  auto by_types = [&](auto L) {
    if (s->cdt == XLBHIP_F32) {
      if (sdt == XLBHIP_F32) return by_order(L, float{}, float{});
      return by_order(L, float{}, _Float16{});
    }
    if (sdt == XLBHIP_F64) return by_order(L, double{}, double{});
    if (sdt == XLBHIP_F32) return by_order(L, double{}, float{});
    return by_order(L, double{}, _Float16{});
  };
  return by_lattice(s->lattice, by_types);
}

static int stats_zero(xlbhip_stats* s) {
  hipStream_t st = s->ctx->stream;
  XLB_HIP(hipMemsetAsync(s->sums.get(), 0, s->cols() * sizeof(double), st));
  XLB_HIP(hipMemsetAsync(s->watch.get(), 0, sizeof(StatsWatch), st));
  s->samples = 0;
  return 0;
}

}  // namespace xlb

extern "C" {

int xlbhip_stats_create(xlbhip_ctx* c, int lattice, int compute_dtype, int nx, int ny, int nz, int keep_mask, int order, const uint32_t exclude[8],
                        xlbhip_stats** out) {
  XLB_REQUIRE(c && out, "null argument");
  XLB_REQUIRE(lattice == XLBHIP_D2Q9 || lattice == XLBHIP_D3Q19 || lattice == XLBHIP_D3Q27, "flow statistics: unknown lattice id %d", lattice);
  XLB_REQUIRE(compute_dtype == XLBHIP_F32 || compute_dtype == XLBHIP_F64, "flow statistics: bad compute dtype %d", compute_dtype);
  XLB_REQUIRE(nx > 0 && ny > 0 && nz > 0 && (size_t)nx * ny * nz < ((size_t)1 << 31), "flow statistics: bad grid %d x %d x %d", nx, ny, nz);
  XLB_REQUIRE(lattice != XLBHIP_D2Q9 || nx == 1, "flow statistics: a 2-D grid is stored as one x plane (%d given)", nx);
  XLB_REQUIRE(keep_mask >= 0 && keep_mask < 8, "flow statistics: the kept axes are a 3-bit set (%d given)", keep_mask);
  XLB_REQUIRE(order == 1 || order == 2, "flow statistics: order must be 1 or 2 (%d given)", order);
  XLB_HIP(hipSetDevice(c->device));
  auto s = std::make_unique<xlbhip_stats>();
  s->ctx = c;
  s->lattice = lattice;
  s->cdt = compute_dtype;
  s->order = order;
  s->plan = stats_plan(nx, ny, nz, keep_mask);
  if (exclude) std::memcpy(s->exclude.bits, exclude, sizeof s->exclude.bits);
  const int d = lattice_d(lattice);
  s->channels = order == 2 ? 3 + d + d * (d + 1) / 2 : 2 + d;
  const size_t scratch_bytes = s->plan.nj > 1 ? (size_t)s->plan.nj * s->cols() * sizeof(double) : 0;
  XLB_REQUIRE(scratch_bytes <= STATS_MAX_SCRATCH_BYTES,
              "flow statistics: %d x %d x %d cells with kept axes %d need %zu bytes of partial sums, more than the %zu the plan allows", nx, ny, nz, keep_mask,
              scratch_bytes, STATS_MAX_SCRATCH_BYTES);
  const hipError_t e = s->sums.alloc(s->cols() * sizeof(double));
  XLB_REQUIRE(e == hipSuccess, "flow statistics: no device memory for %d channels x %lld bins of running sums (%zu bytes): %s", s->channels,
              (long long)s->plan.bins, s->cols() * sizeof(double), hipGetErrorString(e));
  if (scratch_bytes) XLB_HIP(s->scratch.alloc(scratch_bytes));
  XLB_HIP(s->watch.alloc(sizeof(StatsWatch)));
  if (int rc = stats_zero(s.get())) return rc;
  *out = s.release();
  return 0;
}

int xlbhip_stats_destroy(xlbhip_stats* s) {
  if (!s) return 0;
  (void)hipSetDevice(s->ctx->device);
  delete s;  // (hipFree waits for the kernels that still use the buffers)
  return 0;
}

int xlbhip_stats_sample(xlbhip_stats* s, const xlbhip_field* f, const xlbhip_field* bcm) {
  XLB_REQUIRE(s, "null argument");
  XLB_CHECK_POP(f, s->lattice, "flow statistics");
  const StatsPlan& p = s->plan;
  XLB_REQUIRE(f->nx == p.nx && f->ny == p.ny && f->nz == p.nz, "flow statistics: field of %d x %d x %d cells, the object was made for %d x %d x %d", f->nx, f->ny,
              f->nz, p.nx, p.ny, p.nz);
  XLB_REQUIRE(dtype_size(f->dtype) <= dtype_size(s->cdt), "flow statistics: store dtype %d does not fit the compute dtype %d", f->dtype, s->cdt);
  XLB_REQUIRE(!bcm || (bcm->dtype == XLBHIP_U8 && bcm->card == 1), "flow statistics: bc_mask must be a one-component uint8 field");
  XLB_REQUIRE(!bcm || same_grid(bcm, f), "flow statistics: bc_mask of %d x %d x %d cells on a field of %d x %d x %d", bcm ? bcm->nx : 0, bcm ? bcm->ny : 0,
              bcm ? bcm->nz : 0, f->nx, f->ny, f->nz);
  xlbhip_ctx* c = s->ctx;
  XLB_HIP(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  // the last sample's maximum and non-finite count start from zero; bad_total goes on
  XLB_HIP(hipMemsetAsync(s->watch.get(), 0, offsetof(StatsWatch, bad_total), st));
  const unsigned blocks = (unsigned)std::min<int64_t>((p.items + 3) / 4, 2048);
  const int rc = stats_dispatch(s, f->dtype, [&](auto L, auto T, auto S, auto O) {
    using LL = decltype(L);
    using TT = decltype(T);
    using SS = decltype(S);
    auto kernel = (p.keep & STATS_KEEP_Z) ? k_stats_sample<LL, TT, SS, decltype(O)::value, true> : k_stats_sample<LL, TT, SS, decltype(O)::value, false>;
    hipLaunchKernelGGL(kernel, blocks, 256, 0, st, p, static_cast<const SS*>(f->data), f->plane_stride, f->halo,
                       bcm ? static_cast<const uint8_t*>(bcm->data) : nullptr, bcm ? bcm->halo : 0, s->exclude, s->sums.get<double>(),
                       s->scratch.get<double>(), s->watch.get<StatsWatch>());
    XLB_HIP(hipGetLastError());
    return 0;
  });
  if (rc) return rc;
  if (p.nj > 1) {
    const size_t cols = s->cols();
    int bw, jw;
    stats_combine_shape(cols, bw, jw);
    hipLaunchKernelGGL(k_stats_combine, (unsigned)((cols + bw - 1) / bw), 256, 0, st, s->scratch.get<double>(), s->sums.get<double>(), cols, p.nj, bw, jw);
    XLB_HIP(hipGetLastError());
  }
  s->samples += 1;
  return 0;
}

int xlbhip_stats_read(xlbhip_stats* s, int64_t capacity, double* sums, int64_t* samples, double* max_u2, int64_t nonfinite[2]) {
  XLB_REQUIRE(s, "null argument");
  XLB_REQUIRE(!sums || capacity == (int64_t)s->cols(), "xlbhip_stats_read: room for %lld sums, the object holds %d channels x %lld bins", (long long)capacity,
              s->channels, (long long)s->plan.bins);
  xlbhip_ctx* c = s->ctx;
  XLB_HIP(hipSetDevice(c->device));
  StatsWatch w{};
  if (sums) XLB_HIP(hipMemcpyAsync(sums, s->sums.get(), s->cols() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  XLB_HIP(hipMemcpyAsync(&w, s->watch.get(), sizeof w, hipMemcpyDeviceToHost, c->stream));
  XLB_HIP(hipStreamSynchronize(c->stream));
  if (samples) *samples = s->samples;
  if (max_u2) {
    if (s->cdt == XLBHIP_F32) {
      const uint32_t b = (uint32_t)w.umax_bits;
      float v;
      std::memcpy(&v, &b, 4);
      *max_u2 = (double)v;
    } else {
      std::memcpy(max_u2, &w.umax_bits, 8);
    }
  }
  if (nonfinite) {
    nonfinite[0] = (int64_t)w.bad_last;
    nonfinite[1] = (int64_t)w.bad_total;
  }
  return 0;
}

int xlbhip_stats_reset(xlbhip_stats* s) {
  XLB_REQUIRE(s, "null argument");
  XLB_HIP(hipSetDevice(s->ctx->device));
  return stats_zero(s);
}

}  // extern "C"
