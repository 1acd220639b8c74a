// libxlbhip: C-ABI entry points of the context, the fields, the whole-field operators and the halo exchange (the maskers
// live in masker.hip, the stepper in stepper.hip).
// See include/xlbhip.h for the contract and the reference methods each call replaces.
#include <cstring>

#include "api_internal.hpp"
#include "comm.hpp"

namespace xlb {

static thread_local std::string g_err;

void set_error(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
}

int64_t opt(const xlbhip_ctx* c, const char* key, int64_t dflt) {
  auto it = c->opts.find(key);
  return it == c->opts.end() ? dflt : it->second;
}

int lattice_q(int lattice) { return lattice == XLBHIP_D2Q9 ? 9 : (lattice == XLBHIP_D3Q19 ? 19 : (lattice == XLBHIP_D3Q27 ? 27 : 0)); }
int lattice_d(int lattice) { return lattice == XLBHIP_D2Q9 ? 2 : 3; }

static const size_t GUARD_BYTES = 256;

// contents version of a field: globally unique, so a cache keyed on (field address, version) cannot be fooled by a
// new field that recycles a freed one's address
static uint64_t g_version = 0;
void touch(xlbhip_field* f) { f->version = ++g_version; }

int harvest_wait(xlbhip_ctx* c, int slot) {
  if (!c->wait_used[slot]) return 0;
  float ms = 0.f;
  XLB_HIP(hipEventSynchronize(c->ev_w1[slot]));
  XLB_HIP(hipEventElapsedTime(&ms, c->ev_w0[slot], c->ev_w1[slot]));
  c->halo_wait_ms += ms;
  c->halo_waits += 1;
  c->wait_used[slot] = false;
  return 0;
}

template <class L>
static void fill_lattice(int* d, int* q, int32_t* c, double* w, int32_t* op, int32_t* ccv) {
  *d = L::D;
  *q = L::Q;
  for (int l = 0; l < L::Q; ++l) {
    for (int a = 0; a < 3; ++a) c[a * L::Q + l] = L::c(a, l);
    w[l] = L::w(l);
    op[l] = opp<L>(l);
    for (int k = 0; k < 6; ++k) ccv[l * 6 + k] = k < n_pi<L>() ? cc<L>(l, k) : 0;
  }
}

}  // namespace xlb

using namespace xlb;

template <class L, class T>
static int collide_launch(xlbhip_ctx* c, int coll, const xlbhip_field* f, const xlbhip_field* feq, xlbhip_field* fo, double omega) {
  const size_t n = f->cells();
  const T cs = (T)((double)opt(c, "smagorinsky_coef_e6", 170000) * 1e-6);
  if (coll == XLBHIP_BGK) {
    hipLaunchKernelGGL((k_collide<L, T, XLBHIP_BGK>), blocks_for(n), 256, 0, c->stream, view(f), view(feq), view(fo), dims(f), (T)omega, cs);
  } else if (coll == XLBHIP_SMAGORINSKY_LES_BGK) {
    hipLaunchKernelGGL((k_collide<L, T, XLBHIP_SMAGORINSKY_LES_BGK>), blocks_for(n), 256, 0, c->stream, view(f), view(feq), view(fo), dims(f),
                       (T)omega, cs);
  } else if (coll == XLBHIP_REGULARIZED_BGK) {
    hipLaunchKernelGGL((k_collide<L, T, COLL_REGULARIZED>), blocks_for(n), 256, 0, c->stream, view(f), view(feq), view(fo), dims(f), (T)omega, cs);
  } else if (coll == XLBHIP_RECURSIVE_REGULARIZED_BGK) {
    hipLaunchKernelGGL((k_collide<L, T, COLL_REGULARIZED | COLL_RECURSIVE>), blocks_for(n), 256, 0, c->stream, view(f), view(feq), view(fo), dims(f),
                       (T)omega, cs);
  } else {
    if constexpr (L::ID == XLBHIP_D3Q19) {
      XLB_FAIL("Velocity set not supported: D3Q19 has no KBC (reference kbc.py:65-66)");
    } else {
      hipLaunchKernelGGL((k_collide<L, T, XLBHIP_KBC>), blocks_for(n), 256, 0, c->stream, view(f), view(feq), view(fo), dims(f), (T)omega, cs);
    }
  }
  XLB_HIP(hipGetLastError());
  return 0;
}

template <int MODE>
static int velocity_gradient_launch(xlbhip_ctx* c, const xlbhip_field* u, const xlbhip_field* bcm, xlbhip_field* out_a, xlbhip_field* out_b,
                                    const char* what) {
  XLB_REQUIRE(c && u && bcm && out_a && out_b, "%s: null argument", what);
  XLB_REQUIRE(u->card == 3 && (u->dtype == XLBHIP_F32 || u->dtype == XLBHIP_F64), "%s: u must be a (3, nx, ny, nz) fp32 / fp64 field", what);
  XLB_REQUIRE(u->halo == 0, "%s: fields with ghost planes are not supported (single-rank post-processing, like the reference)", what);
  XLB_REQUIRE(bcm->dtype == XLBHIP_U8 && bcm->card == 1 && same_grid(bcm, u) && bcm->halo == 0, "%s: bad bc_mask field", what);
  XLB_REQUIRE(out_a->card == (MODE == 0 ? 3 : 1) && out_b->card == 1 && is_float(out_a->dtype) && is_float(out_b->dtype) &&
                  same_grid(out_a, u) && same_grid(out_b, u) && out_a->halo == 0 && out_b->halo == 0,
              "%s: bad output fields", what);
  const size_t n = u->cells();
  if (u->dtype == XLBHIP_F32)
    hipLaunchKernelGGL((k_velocity_gradient<float, MODE>), blocks_for(n), 256, 0, c->stream, view(u), view(bcm), view(out_a), view(out_b), dims(u));
  else
    hipLaunchKernelGGL((k_velocity_gradient<double, MODE>), blocks_for(n), 256, 0, c->stream, view(u), view(bcm), view(out_a), view(out_b), dims(u));
  XLB_HIP(hipGetLastError());
  return 0;
}

extern "C" {

const char* xlbhip_last_error(void) { return g_err.c_str(); }

int xlbhip_create(int device, xlbhip_ctx** out) {
  XLB_REQUIRE(out, "out is null");
  int n = 0;
  XLB_HIP(hipGetDeviceCount(&n));
  XLB_REQUIRE(n > 0, "no HIP device visible");
  XLB_REQUIRE(device >= 0 && device < n, "device %d out of range (have %d)", device, n);
  XLB_HIP(hipSetDevice(device));
  xlbhip_ctx* c = new xlbhip_ctx();
  c->device = device;
  XLB_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  // the halo stream outranks the compute stream: its small kernels / copies must not queue behind the interior launch
  int prio_low = 0, prio_high = 0;
  XLB_HIP(hipDeviceGetStreamPriorityRange(&prio_low, &prio_high));
  XLB_HIP(hipStreamCreateWithPriority(&c->comm_stream, hipStreamNonBlocking, prio_high));
  XLB_HIP(hipEventCreate(&c->ev_a));
  XLB_HIP(hipEventCreate(&c->ev_b));
  XLB_HIP(hipEventCreateWithFlags(&c->ev_edge, hipEventDisableTiming));
  XLB_HIP(hipEventCreateWithFlags(&c->ev_halo, hipEventDisableTiming));
  hipDeviceProp_t p;
  XLB_HIP(hipGetDeviceProperties(&p, device));
  c->compute_units = p.multiProcessorCount;
  // defaults of the tuning knobs
  c->opts["vec"] = 0;              // cells per thread: 0 = auto (1), or 1 / 2 / 4
  c->opts["nt_store"] = 1;         // non-temporal stores in the fused kernel
  c->opts["nt_load"] = 1;          // 1: nt loads for the c_z == 0 directions (+1.8 %), 3: for all (slower; D3Q19 BGK tuning variants only)
  c->opts["plane_pad_bytes"] = 4352;  // de-alias the q population planes
  c->opts["block_threads"] = 256;
  c->opts["xcd_swizzle"] = 0;      // blocks of one row on one XCD (see step_kernel.hpp)
  c->opts["block_tz"] = 0;         // threads along z per block (0 = a whole row when it fits)
  c->opts["overlap"] = 1;          // halo exchange overlapped with the interior kernel
  c->opts["smagorinsky_coef_e6"] = 170000;  // Smagorinsky constant x 1e6 for the STAND-ALONE collision operator (0.17)
  c->opts["fuse2"] = 1;            // xlbhip_run: two steps per pass (step2_kernel.hpp): 0 never, 1 where eligible and the grid fills the chip, 2 wherever eligible
  c->opts["fuse2_xseg"] = 0;       // x segments per tile column in the two-step kernel (0 = auto: 4, fewer for short domains)
  c->opts["fuse2_clean"] = 1;      // two-step kernel with BCs: work items without boundary cells run the BC-free body (same launch)
  c->opts["fuse2_cus"] = 0;        // CUs the chip-filling rule of fuse2 = 1 assumes (0 = the device's; tests of the rule)
  c->opts["fuse2_strips"] = 1;     // two-step kernel (D3Q19): halo columns of phase A from the fields' strip buffers (step2_kernel.hpp): 0 never,
                                   // 1 = for steppers with boundary conditions (where they pay), 2 = always
  c->opts["fuse2_rowmap"] = 0;     // measurement: 1 = the BC kernel's bodies with row-aligned lanes and NO strip buffers (fuse2_strips must be 0)
  c->opts["fast_bgk"] = 0;         // two-step kernel: 1 = tolerance-graded fast BGK body (rounding-level differences; +2-4 %)
  c->opts["exact_math"] = 0;       // 1: bit-exact builds only (fp64 KBC otherwise uses the tolerance-graded fast collision, cell.hpp kbc_fast)
  c->opts["external_halo"] = 0;    // 1: the caller fills the ghost planes before every step (host-staged transports, tests)
  c->opts["halo_telemetry"] = 1;   // slab runs: time the compute stream's wait for the halo event (xlbhip_comm_stats)
  c->opts["ipc_copy"] = 1;         // ipc transport: 1 = one pull kernel per exchange (8 blocks per plane, no LDS: hidden behind the interior launch),
                                   // 0 = plane-sized hipMemcpyAsync pulls (copy engines; ~40 us per call on a shared device: profiles/r03/ipc_transport.md)
  c->opts["ipc_timeout_ms"] = 180000;  // ipc transport: bound of every device-side / host-side wait for a neighbour (ranks reach their first
                                       // exchange as unevenly as their set-up takes: callers should put a barrier in front of the first run)
  c->opts["halo_skip"] = 0;        // 1: MEASUREMENT ONLY — the slab protocol's launches without moving any ghost plane (wrong results)
  c->opts["comm_self_test"] = 0;   // 1: a one-rank RCCL communicator also runs the all-reduce of comm_all_min (tests)
  *out = c;
  return 0;
}

int xlbhip_destroy(xlbhip_ctx* c) {
  if (!c) return 0;
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();
  xlbhip_comm_destroy(c);
  (void)hipEventDestroy(c->ev_a);
  (void)hipEventDestroy(c->ev_b);
  (void)hipEventDestroy(c->ev_edge);
  (void)hipEventDestroy(c->ev_halo);
  for (int i = 0; i < xlbhip_ctx::WAIT_RING; ++i) {
    if (c->ev_w0[i]) (void)hipEventDestroy(c->ev_w0[i]);
    if (c->ev_w1[i]) (void)hipEventDestroy(c->ev_w1[i]);
  }
  (void)hipStreamDestroy(c->stream);
  (void)hipStreamDestroy(c->comm_stream);
  delete c;
  return 0;
}

int xlbhip_sync(xlbhip_ctx* c) {
  XLB_REQUIRE(c, "ctx is null");
  XLB_HIP(hipStreamSynchronize(c->comm_stream));
  XLB_HIP(hipStreamSynchronize(c->stream));
  return comm_check(c);
}

int xlbhip_device_info(xlbhip_ctx* c, char* name, int name_len, int* cus, uint64_t* hbm) {
  XLB_REQUIRE(c, "ctx is null");
  hipDeviceProp_t p;
  XLB_HIP(hipGetDeviceProperties(&p, c->device));
  if (name && name_len > 0) {
    snprintf(name, name_len, "%s (%s)", p.name, p.gcnArchName);
  }
  if (cus) *cus = p.multiProcessorCount;
  if (hbm) *hbm = p.totalGlobalMem;
  return 0;
}

int xlbhip_set_option(xlbhip_ctx* c, const char* key, int64_t value) {
  XLB_REQUIRE(c && key, "null argument");
  auto it = c->opts.find(key);
  XLB_REQUIRE(it != c->opts.end(), "unknown option '%s'", key);
  it->second = value;
  return 0;
}
int xlbhip_get_option(xlbhip_ctx* c, const char* key, int64_t* value) {
  XLB_REQUIRE(c && key && value, "null argument");
  auto it = c->opts.find(key);
  XLB_REQUIRE(it != c->opts.end(), "unknown option '%s'", key);
  *value = it->second;
  return 0;
}

int xlbhip_lattice_info(int lattice, int* d, int* q, int32_t* c, double* w, int32_t* op, int32_t* ccv) {
  XLB_REQUIRE(d && q && c && w && op && ccv, "null output");
  return by_lattice(lattice, [&](auto L) {
    fill_lattice<decltype(L)>(d, q, c, w, op, ccv);
    return 0;
  });
}

// ---- fields ---------------------------------------------------------------------------
int xlbhip_field_create(xlbhip_ctx* c, int card, int nx, int ny, int nz, int dtype, int halo, double fill, xlbhip_field** out) {
  XLB_REQUIRE(c && out, "null argument");
  XLB_REQUIRE(card >= 1 && nx >= 1 && ny >= 1 && nz >= 1, "bad field shape (%d,%d,%d,%d)", card, nx, ny, nz);
  XLB_REQUIRE(halo >= 0 && halo <= 2, "halo must be 0, 1 or 2");
  XLB_REQUIRE(dtype_size(dtype) > 0, "bad dtype %d", dtype);
  XLB_REQUIRE(dtype != XLBHIP_MISSING || card <= 32, "missing_mask cardinality %d > 32", card);
  XLB_HIP(hipSetDevice(c->device));
  xlbhip_field* f = new xlbhip_field();
  f->ctx = c;
  f->card = card;
  f->nx = nx;
  f->ny = ny;
  f->nz = nz;
  f->halo = halo;
  f->dtype = dtype;
  f->planes = dtype == XLBHIP_MISSING ? 1 : card;
  const size_t es = dtype_size(dtype);
  size_t stride = f->cells_with_halo();
  if (f->planes > 1) {
    // pad the plane stride (multiple of 16 B keeps vector alignment) so that the q planes
    // of one cell do not land on the same HBM channel when the extent is a power of two
    size_t pad = (size_t)opt(c, "plane_pad_bytes", 0) / es;
    stride += pad;
  }
  const size_t align_elems = 256 / es;  // keep every plane 256-B aligned
  stride = (stride + align_elems - 1) / align_elems * align_elems;
  f->plane_stride = stride;
  f->alloc_bytes = f->planes * stride * es + 2 * GUARD_BYTES;
  hipError_t e = hipMalloc(&f->base, f->alloc_bytes);
  if (e != hipSuccess) {
    delete f;
    XLB_FAIL("hipMalloc(%zu bytes) failed: %s", f->alloc_bytes, hipGetErrorString(e));
  }
  f->data = static_cast<char*>(f->base) + GUARD_BYTES;
  touch(f);  // a fresh contents version: no cache entry of a freed field at this address can match
  *out = f;
  if (dtype == XLBHIP_MISSING) {
    XLB_REQUIRE(fill == 0.0, "missing_mask fill must be 0");
  }
  return xlbhip_field_fill(f, fill);
}

int xlbhip_field_destroy(xlbhip_field* f) {
  if (!f) return 0;
  (void)hipSetDevice(f->ctx->device);
  (void)hipStreamSynchronize(f->ctx->stream);
  (void)hipStreamSynchronize(f->ctx->comm_stream);
  comm_forget_buffer(f->ctx, f->base);
  if (f->strips) (void)hipFree(f->strips);
  (void)hipFree(f->base);
  delete f;
  return 0;
}

int xlbhip_field_fill(xlbhip_field* f, double v) {
  XLB_REQUIRE(f, "field is null");
  touch(f);
  hipStream_t st = f->ctx->stream;
  if (v == 0.0) {
    XLB_HIP(hipMemsetAsync(f->base, 0, f->alloc_bytes, st));
    return 0;
  }
  const size_t n = f->planes * f->plane_stride;
  switch (f->dtype) {
    case XLBHIP_F64: hipLaunchKernelGGL(k_fill<double>, blocks_capped(n), 256, 0, st, (double*)f->data, n, v); break;
    case XLBHIP_F32: hipLaunchKernelGGL(k_fill<float>, blocks_capped(n), 256, 0, st, (float*)f->data, n, (float)v); break;
    case XLBHIP_F16: hipLaunchKernelGGL(k_fill<_Float16>, blocks_capped(n), 256, 0, st, (_Float16*)f->data, n, (_Float16)v); break;
    case XLBHIP_U8: hipLaunchKernelGGL(k_fill<uint8_t>, blocks_capped(n), 256, 0, st, (uint8_t*)f->data, n, (uint8_t)v); break;
    case XLBHIP_BOOL: hipLaunchKernelGGL(k_fill<uint8_t>, blocks_capped(n), 256, 0, st, (uint8_t*)f->data, n, (uint8_t)(v != 0.0)); break;
    default: XLB_FAIL("cannot fill dtype %d with a non-zero value", f->dtype);
  }
  XLB_HIP(hipGetLastError());
  return 0;
}

int xlbhip_field_copy(xlbhip_field* dst, const xlbhip_field* src) {
  XLB_REQUIRE(dst && src, "null field");
  XLB_REQUIRE(dst->dtype == src->dtype && dst->card == src->card && same_grid(dst, src) && dst->halo == src->halo &&
                  dst->plane_stride == src->plane_stride,
              "field_copy: layouts differ");
  touch(dst);
  XLB_HIP(hipMemcpyAsync(dst->base, src->base, src->alloc_bytes, hipMemcpyDeviceToDevice, dst->ctx->stream));
  return 0;
}

int xlbhip_field_copy_kernel(xlbhip_field* dst, const xlbhip_field* src, int bytes_per_lane) {
  XLB_REQUIRE(dst && src, "null field");
  XLB_REQUIRE(dst->alloc_bytes == src->alloc_bytes && dst != src, "field_copy_kernel: layouts differ");
  XLB_REQUIRE(bytes_per_lane == 4 || bytes_per_lane == 16, "bytes_per_lane must be 4 or 16");
  const size_t bytes = src->planes * src->plane_stride * dtype_size(src->dtype);
  XLB_REQUIRE(bytes % 16 == 0, "field size not a multiple of 16 bytes");
  touch(dst);
  hipStream_t st = dst->ctx->stream;
  if (bytes_per_lane == 4) {
    const size_t n = bytes / 4;
    hipLaunchKernelGGL(k_copy<uint32_t>, blocks_capped(n), 256, 0, st, (const uint32_t*)src->data, (uint32_t*)dst->data, n);
  } else {
    const size_t n = bytes / 16;
    hipLaunchKernelGGL(k_copy<u32x4>, blocks_capped(n), 256, 0, st, (const u32x4*)src->data, (u32x4*)dst->data, n);
  }
  XLB_HIP(hipGetLastError());
  return 0;
}

int xlbhip_field_touch(xlbhip_field* f) {
  XLB_REQUIRE(f, "field is null");
  touch(f);
  return 0;
}

int xlbhip_mem_info(xlbhip_ctx* c, uint64_t* free_bytes, uint64_t* total_bytes) {
  XLB_REQUIRE(c, "ctx is null");
  XLB_HIP(hipSetDevice(c->device));
  size_t fr = 0, tot = 0;
  XLB_HIP(hipMemGetInfo(&fr, &tot));
  if (free_bytes) *free_bytes = fr;
  if (total_bytes) *total_bytes = tot;
  return 0;
}

int xlbhip_field_info(const xlbhip_field* f, int* card, int* nx, int* ny, int* nz, int* dtype, int* halo, uint64_t* ps, void** ptr) {
  XLB_REQUIRE(f, "field is null");
  if (card) *card = f->card;
  if (nx) *nx = f->nx;
  if (ny) *ny = f->ny;
  if (nz) *nz = f->nz;
  if (dtype) *dtype = f->dtype;
  if (halo) *halo = f->halo;
  if (ps) *ps = f->plane_stride;
  if (ptr) *ptr = f->data;
  return 0;
}

int xlbhip_field_upload(xlbhip_field* f, const void* host, size_t bytes) {
  XLB_REQUIRE(f && host, "null argument");
  touch(f);
  hipStream_t st = f->ctx->stream;
  const size_t n = f->cells();
  if (f->dtype == XLBHIP_MISSING) {
    XLB_REQUIRE(bytes == n * f->card, "upload size %zu != %zu", bytes, n * f->card);
    uint8_t* tmp = nullptr;
    XLB_HIP(hipMalloc(&tmp, bytes));
    XLB_HIP(hipMemcpyAsync(tmp, host, bytes, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_pack_missing, blocks_for(n), 256, 0, st, tmp, (uint32_t*)f->data, f->card, dims(f), f->halo);
    XLB_HIP(hipGetLastError());
    XLB_HIP(hipStreamSynchronize(st));
    XLB_HIP(hipFree(tmp));
    return 0;
  }
  const size_t es = dtype_size(f->dtype);
  XLB_REQUIRE(bytes == n * f->card * es, "upload size %zu != %zu", bytes, n * f->card * es);
  for (int l = 0; l < f->card; ++l) {
    char* d = static_cast<char*>(f->data) + ((size_t)l * f->plane_stride + (size_t)f->halo * f->ny * f->nz) * es;
    XLB_HIP(hipMemcpyAsync(d, static_cast<const char*>(host) + (size_t)l * n * es, n * es, hipMemcpyHostToDevice, st));
  }
  XLB_HIP(hipStreamSynchronize(st));  // the host buffer may be reused by the caller
  return 0;
}

int xlbhip_field_download(const xlbhip_field* f, void* host, size_t bytes) {
  XLB_REQUIRE(f && host, "null argument");
  hipStream_t st = f->ctx->stream;
  const size_t n = f->cells();
  XLB_HIP(hipStreamSynchronize(f->ctx->comm_stream));
  if (f->dtype == XLBHIP_MISSING) {
    XLB_REQUIRE(bytes == n * f->card, "download size %zu != %zu", bytes, n * f->card);
    uint8_t* tmp = nullptr;
    XLB_HIP(hipMalloc(&tmp, bytes));
    hipLaunchKernelGGL(k_unpack_missing, blocks_for(n), 256, 0, st, (const uint32_t*)f->data, tmp, f->card, dims(f), f->halo);
    XLB_HIP(hipGetLastError());
    XLB_HIP(hipMemcpyAsync(host, tmp, bytes, hipMemcpyDeviceToHost, st));
    XLB_HIP(hipStreamSynchronize(st));
    XLB_HIP(hipFree(tmp));
    return 0;
  }
  const size_t es = dtype_size(f->dtype);
  XLB_REQUIRE(bytes == n * f->card * es, "download size %zu != %zu", bytes, n * f->card * es);
  for (int l = 0; l < f->card; ++l) {
    const char* s = static_cast<const char*>(f->data) + ((size_t)l * f->plane_stride + (size_t)f->halo * f->ny * f->nz) * es;
    XLB_HIP(hipMemcpyAsync(static_cast<char*>(host) + (size_t)l * n * es, s, n * es, hipMemcpyDeviceToHost, st));
  }
  XLB_HIP(hipStreamSynchronize(st));
  return 0;
}

int xlbhip_field_plane_download(const xlbhip_field* f, int population, int storage_plane, void* host, size_t bytes) {
  XLB_REQUIRE(f && host, "null argument");
  // (the bit-packed missing_mask has ONE device plane of uint32 bit-sets: population 0)
  XLB_REQUIRE(population >= 0 && population < f->planes && storage_plane >= 0 && storage_plane < f->nx + 2 * f->halo,
              "plane (%d, %d) out of range", population, storage_plane);
  const size_t es = dtype_size(f->dtype), plane = (size_t)f->ny * f->nz;
  XLB_REQUIRE(bytes == plane * es, "plane size %zu != %zu", bytes, plane * es);
  const char* s = static_cast<const char*>(f->data) + ((size_t)population * f->plane_stride + (size_t)storage_plane * plane) * es;
  XLB_HIP(hipMemcpyAsync(host, s, bytes, hipMemcpyDeviceToHost, f->ctx->stream));
  XLB_HIP(hipStreamSynchronize(f->ctx->stream));
  return 0;
}

int xlbhip_field_plane_upload(xlbhip_field* f, int population, int storage_plane, const void* host, size_t bytes) {
  XLB_REQUIRE(f && host, "null argument");
  // (the bit-packed missing_mask has ONE device plane of uint32 bit-sets: population 0)
  XLB_REQUIRE(population >= 0 && population < f->planes && storage_plane >= 0 && storage_plane < f->nx + 2 * f->halo,
              "plane (%d, %d) out of range", population, storage_plane);
  const size_t es = dtype_size(f->dtype), plane = (size_t)f->ny * f->nz;
  XLB_REQUIRE(bytes == plane * es, "plane size %zu != %zu", bytes, plane * es);
  touch(f);
  char* d = static_cast<char*>(f->data) + ((size_t)population * f->plane_stride + (size_t)storage_plane * plane) * es;
  XLB_HIP(hipMemcpyAsync(d, host, bytes, hipMemcpyHostToDevice, f->ctx->stream));
  XLB_HIP(hipStreamSynchronize(f->ctx->stream));
  return 0;
}

// ---- whole-field operators --------------------------------------------------------------
int xlbhip_stream(xlbhip_ctx* c, int lattice, const xlbhip_field* src, xlbhip_field* dst) {
  XLB_REQUIRE(c, "ctx is null");
  XLB_REQUIRE(src && dst && src->card == lattice_q(lattice) && dst->card == src->card && same_grid(src, dst),
              "stream: field shapes do not match the lattice");
  XLB_REQUIRE(src->dtype != XLBHIP_MISSING && dst->dtype == src->dtype, "stream: dtype mismatch");
  XLB_REQUIRE(src != dst, "stream: f_0 and f_1 must be different fields");
  touch(dst);
  const size_t n = src->cells();
  return by_lattice(lattice, [&](auto L) {
    hipLaunchKernelGGL(k_stream<decltype(L)>, blocks_for(n), 256, 0, c->stream, view(src), view(dst), dims(src));
    XLB_HIP(hipGetLastError());
    return 0;
  });
}

int xlbhip_equilibrium(xlbhip_ctx* c, int lattice, int cdt, const xlbhip_field* rho, const xlbhip_field* u, xlbhip_field* f) {
  XLB_REQUIRE(c, "ctx is null");
  XLB_CHECK_POP(f, lattice, "equilibrium");
  XLB_REQUIRE(rho && u && rho->card == 1 && u->card == lattice_d(lattice) && same_grid(rho, f) && same_grid(u, f) &&
                  is_float(rho->dtype) && is_float(u->dtype),
              "equilibrium: rho must be (1,...) and u (d,...) float fields on f's grid");
  XLB_REQUIRE(cdt == XLBHIP_F32 || cdt == XLBHIP_F64, "bad compute dtype %d", cdt);
  touch(f);
  const size_t n = f->cells();
  return by_lattice(lattice, [&](auto L) {
    return by_compute(cdt, [&](auto T) {
      hipLaunchKernelGGL((k_equilibrium<decltype(L), decltype(T)>), blocks_for(n), 256, 0, c->stream, view(rho), view(u), view(f), dims(f));
      XLB_HIP(hipGetLastError());
      return 0;
    });
  });
}

int xlbhip_macroscopic(xlbhip_ctx* c, int lattice, int cdt, const xlbhip_field* f, xlbhip_field* rho, xlbhip_field* u) {
  XLB_REQUIRE(c, "ctx is null");
  XLB_CHECK_POP(f, lattice, "macroscopic");
  XLB_REQUIRE(!rho || (rho->card == 1 && same_grid(rho, f) && is_float(rho->dtype)), "macroscopic: bad rho field");
  XLB_REQUIRE(!u || (u->card == lattice_d(lattice) && same_grid(u, f) && is_float(u->dtype)), "macroscopic: bad u field");
  XLB_REQUIRE(cdt == XLBHIP_F32 || cdt == XLBHIP_F64, "bad compute dtype %d", cdt);
  const size_t n = f->cells();
  return by_lattice(lattice, [&](auto L) {
    return by_compute(cdt, [&](auto T) {
      hipLaunchKernelGGL((k_macroscopic<decltype(L), decltype(T)>), blocks_for(n), 256, 0, c->stream, view(f), view(rho), view(u), dims(f));
      XLB_HIP(hipGetLastError());
      return 0;
    });
  });
}

int xlbhip_momentum_transfer(xlbhip_ctx* c, int lattice, int cdt, const xlbhip_bc_desc* bc, const xlbhip_field* f_0, const xlbhip_field* bcm,
                             const xlbhip_field* miss, double force_out[3]) {
  XLB_REQUIRE(c && bc && force_out, "null argument");
  XLB_CHECK_POP(f_0, lattice, "momentum_transfer(f_0)");
  XLB_REQUIRE(bcm && bcm->dtype == XLBHIP_U8 && bcm->card == 1 && same_grid(bcm, f_0) && bcm->halo == f_0->halo, "momentum_transfer: bad bc_mask field");
  XLB_REQUIRE(miss && miss->dtype == XLBHIP_MISSING && same_grid(miss, f_0) && miss->halo == f_0->halo, "momentum_transfer: needs the missing_mask field");
  XLB_REQUIRE(bc->kind == XLBHIP_BC_HALFWAY_BB || bc->kind == XLBHIP_BC_FULLWAY_BB,
              "momentum_transfer: the no-slip BC must be a halfway or fullway bounce-back (kind %d given)", bc->kind);
  XLB_REQUIRE(cdt == XLBHIP_F32 || cdt == XLBHIP_F64, "bad compute dtype %d", cdt);
  DeviceBuf dforce;
  XLB_HIP(dforce.alloc(3 * sizeof(double)));
  XLB_HIP(hipMemsetAsync(dforce.get(), 0, 3 * sizeof(double), c->stream));
  const size_t n = f_0->cells();
  const int wall = bc->kind == XLBHIP_BC_HALFWAY_BB ? 1 : 0;
  const int rc = by_lattice(lattice, [&](auto L) {
    return by_compute(cdt, [&](auto T) {
      hipLaunchKernelGGL((k_momentum_transfer<decltype(L), decltype(T)>), blocks_for(n), BC_BLOCK, 0, c->stream, view(f_0), view(bcm), view(miss), dims(f_0),
                         bc->id, bc_values<decltype(T)>(bc->values), wall, dforce.get<double>());
      XLB_HIP(hipGetLastError());
      return 0;
    });
  });
  if (rc) return rc;
  hipError_t e = hipMemcpyAsync(force_out, dforce.get(), 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  XLB_REQUIRE(e == hipSuccess, "momentum_transfer: %s", hipGetErrorString(e));
  return 0;
}

int xlbhip_grid_to_point(xlbhip_ctx* c, const xlbhip_field* grid, int64_t n, const float* points, void* values) {
  XLB_REQUIRE(c && grid && (n == 0 || (points && values)), "grid_to_point: null argument");
  XLB_REQUIRE((grid->dtype == XLBHIP_F32 || grid->dtype == XLBHIP_F64) && grid->halo == 0, "grid_to_point: fp32 / fp64 field without ghost planes");
  if (n == 0) return 0;
  // every point needs its surrounding cube inside the field (the reference does not check; an out-of-range point reads
  // out of bounds there)
  for (int64_t i = 0; i < n; ++i)
    for (int a = 0; a < 3; ++a) {
      const float p = points[3 * i + a];
      const int ext = a == 0 ? grid->nx : (a == 1 ? grid->ny : grid->nz);
      XLB_REQUIRE(p >= 0.0f && (int)p + 1 <= ext - 1, "grid_to_point: point %lld (%g along axis %d) needs cells outside the field", (long long)i,
                  (double)p, a);
    }
  const size_t es = dtype_size(grid->dtype);
  float* dp = nullptr;
  void* dv = nullptr;
  XLB_HIP(hipMalloc(&dp, (size_t)n * 3 * sizeof(float)));
  hipError_t e = hipMalloc(&dv, (size_t)n * es);
  if (e != hipSuccess) {
    (void)hipFree(dp);
    XLB_FAIL("grid_to_point: %s", hipGetErrorString(e));
  }
  e = hipMemcpyAsync(dp, points, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    if (grid->dtype == XLBHIP_F32)
      hipLaunchKernelGGL((k_grid_to_point<float>), blocks_for((size_t)n), 256, 0, c->stream, view(grid), dims(grid), dp, static_cast<float*>(dv), n);
    else
      hipLaunchKernelGGL((k_grid_to_point<double>), blocks_for((size_t)n), 256, 0, c->stream, view(grid), dims(grid), dp, static_cast<double*>(dv), n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(values, dv, (size_t)n * es, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(dp);
  (void)hipFree(dv);
  XLB_REQUIRE(e == hipSuccess, "grid_to_point: %s", hipGetErrorString(e));
  return 0;
}

int xlbhip_vorticity(xlbhip_ctx* c, const xlbhip_field* u, const xlbhip_field* bcm, xlbhip_field* vorticity, xlbhip_field* magnitude) {
  return velocity_gradient_launch<0>(c, u, bcm, vorticity, magnitude, "vorticity");
}

int xlbhip_q_criterion(xlbhip_ctx* c, const xlbhip_field* u, const xlbhip_field* bcm, xlbhip_field* norm_mu, xlbhip_field* q) {
  return velocity_gradient_launch<1>(c, u, bcm, norm_mu, q, "q_criterion");
}

int xlbhip_second_moment(xlbhip_ctx* c, int lattice, int cdt, const xlbhip_field* f, xlbhip_field* pi) {
  XLB_REQUIRE(c, "ctx is null");
  XLB_CHECK_POP(f, lattice, "second_moment");
  const int nt = lattice_d(lattice) * (lattice_d(lattice) + 1) / 2;
  XLB_REQUIRE(pi && pi->card == nt && same_grid(pi, f) && is_float(pi->dtype), "second_moment: pi must be a (%d,...) float field", nt);
  XLB_REQUIRE(cdt == XLBHIP_F32 || cdt == XLBHIP_F64, "bad compute dtype %d", cdt);
  const size_t n = f->cells();
  return by_lattice(lattice, [&](auto L) {
    return by_compute(cdt, [&](auto T) {
      hipLaunchKernelGGL((k_second_moment<decltype(L), decltype(T)>), blocks_for(n), 256, 0, c->stream, view(f), view(pi), dims(f));
      XLB_HIP(hipGetLastError());
      return 0;
    });
  });
}

int xlbhip_collide(xlbhip_ctx* c, int lattice, int coll, int cdt, const xlbhip_field* f, const xlbhip_field* feq, xlbhip_field* fo,
                   double omega) {
  XLB_REQUIRE(c, "ctx is null");
  XLB_CHECK_POP(f, lattice, "collide(f)");
  XLB_CHECK_POP(feq, lattice, "collide(feq)");
  XLB_CHECK_POP(fo, lattice, "collide(fout)");
  XLB_REQUIRE(same_grid(f, feq) && same_grid(f, fo), "collide: grids differ");
  XLB_REQUIRE(coll >= XLBHIP_BGK && coll <= XLBHIP_RECURSIVE_REGULARIZED_BGK, "unknown collision %d", coll);
  XLB_REQUIRE(cdt == XLBHIP_F32 || cdt == XLBHIP_F64, "bad compute dtype %d", cdt);
  touch(fo);
  return by_lattice(lattice, [&](auto L) {
    return by_compute(cdt, [&](auto T) { return collide_launch<decltype(L), decltype(T)>(c, coll, f, feq, fo, omega); });
  });
}

int xlbhip_apply_bc(xlbhip_ctx* c, int lattice, int cdt, const xlbhip_bc_desc* bc, const xlbhip_field* f_pre, xlbhip_field* f_post,
                    const xlbhip_field* bcm, const xlbhip_field* miss) {
  return xlbhip_apply_bc_profile(c, lattice, cdt, bc, f_pre, f_post, bcm, miss, 0, nullptr, nullptr);
}

int xlbhip_apply_bc_profile(xlbhip_ctx* c, int lattice, int cdt, const xlbhip_bc_desc* bc, const xlbhip_field* f_pre, xlbhip_field* f_post,
                            const xlbhip_field* bcm, const xlbhip_field* miss, int64_t n_prof, const uint32_t* storage_cells,
                            const double* values) {
  XLB_REQUIRE(c && bc, "null argument");
  XLB_CHECK_POP(f_pre, lattice, "bc(f_pre)");
  XLB_CHECK_POP(f_post, lattice, "bc(f_post)");
  XLB_REQUIRE(bcm && bcm->dtype == XLBHIP_U8 && bcm->card == 1 && same_grid(bcm, f_post), "bc: bad bc_mask field");
  XLB_REQUIRE(same_grid(f_pre, f_post), "bc: grids differ");
  touch(f_post);
  XLB_REQUIRE(bc->id >= 1 && bc->id <= 255, "bc id %d out of range", bc->id);
  XLB_REQUIRE(bc_is_known(bc->kind) && bc->kind != XLBHIP_BC_HALFWAY_BB_PROFILE, "unknown bc kind %d (wall-velocity tables live in the stepper)", bc->kind);
  XLB_REQUIRE(!bc_is_hybrid(bc->kind) || (lattice_d(lattice) == 3 && bc->values[4] == 0.0),
              "HybridBC as a stand-alone operator: 3-D lattices, without mesh distances (those live in the stepper: xlbhip_stepper_set_bc_distances)");
  if (bc_reads_missing(bc->kind))
    XLB_REQUIRE(miss && miss->dtype == XLBHIP_MISSING && same_grid(miss, f_post), "bc: this boundary condition needs a missing_mask field");
  XLB_REQUIRE(cdt == XLBHIP_F32 || cdt == XLBHIP_F64, "bad compute dtype %d", cdt);
  const size_t n = f_post->cells();
  // per-cell prescribed values (sorted by storage cell, in the compute dtype): uploaded for this call only — the stand-alone
  // operator is not on the hot path
  std::vector<uint32_t> keys;
  std::vector<char> image;
  DeviceScratch scratch(c->stream);  // (declared after the host vectors: it drains the stream before they die)
  uint32_t* dk = nullptr;
  char* dv = nullptr;
  if (n_prof > 0) {
    XLB_REQUIRE(storage_cells && values, "null profile table");
    XLB_REQUIRE(bc_is_zouhe_family(bc->kind), "profiles belong to Zou-He / Regularized BCs");
    std::vector<std::pair<uint32_t, int64_t>> order((size_t)n_prof);
    for (int64_t i = 0; i < n_prof; ++i) order[(size_t)i] = {storage_cells[i], i};
    std::sort(order.begin(), order.end());
    keys.resize((size_t)n_prof);
    std::vector<double> v((size_t)n_prof * 3);
    for (int64_t i = 0; i < n_prof; ++i) {
      keys[(size_t)i] = order[(size_t)i].first;
      for (int a = 0; a < 3; ++a) v[(size_t)i * 3 + a] = values[order[(size_t)i].second * 3 + a];
    }
    image = compute_image(cdt, v);
    XLB_HIP(scratch.alloc(&dk, keys.size() * sizeof(uint32_t)));
    XLB_HIP(scratch.alloc(&dv, image.size()));
    XLB_HIP(hipMemcpyAsync(dk, keys.data(), keys.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    XLB_HIP(hipMemcpyAsync(dv, image.data(), image.size(), hipMemcpyHostToDevice, c->stream));
  }
  const int np = (int)n_prof;
  return by_lattice(lattice, [&](auto L) {
    return by_compute(cdt, [&](auto T) {
      using TT = decltype(T);
      BcValues<TT> vals = bc_values<TT>(bc->values);
      if (np > 0) vals.v[PROF_FLAG] = TT(1);  // prescribed values come from the table (cell.hpp: wall_velocity)
      hipLaunchKernelGGL((k_apply_bc<decltype(L), TT>), blocks_for(n), BC_BLOCK, 0, c->stream, bc->id, bc->kind, vals, view(f_pre), view(f_post),
                         view(bcm), view(miss), dims(f_post), dk, reinterpret_cast<const TT*>(dv), np);
      XLB_HIP(hipGetLastError());
      return 0;
    });
  });
}

int xlbhip_field_gather(const xlbhip_field* f, int64_t n, const uint32_t* cells, void* out, size_t bytes) {
  XLB_REQUIRE(f && (n == 0 || (cells && out)), "field_gather: null argument");
  XLB_REQUIRE(f->dtype != XLBHIP_MISSING, "field_gather: not for the bit-packed missing_mask");
  const size_t es = dtype_size(f->dtype);
  XLB_REQUIRE(bytes == (size_t)n * f->card * es, "field_gather: output size %zu != %zu", bytes, (size_t)n * f->card * es);
  if (n == 0) return 0;
  for (int64_t i = 0; i < n; ++i) XLB_REQUIRE(cells[i] < f->cells(), "field_gather: cell %u outside the field", cells[i]);
  hipStream_t st = f->ctx->stream;
  DeviceScratch scratch(st);
  uint32_t* dc = nullptr;
  char* dout = nullptr;
  XLB_HIP(scratch.alloc(&dc, (size_t)n * sizeof(uint32_t)));
  XLB_HIP(scratch.alloc(&dout, bytes));
  XLB_HIP(hipMemcpyAsync(dc, cells, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  const size_t ghost = (size_t)f->halo * f->ny * f->nz;
  switch (es) {
    case 8: hipLaunchKernelGGL(k_gather<uint64_t>, blocks_for((size_t)n), 256, 0, st, (const uint64_t*)f->data, f->plane_stride, ghost, f->card, dc, n, (uint64_t*)dout); break;
    case 4: hipLaunchKernelGGL(k_gather<uint32_t>, blocks_for((size_t)n), 256, 0, st, (const uint32_t*)f->data, f->plane_stride, ghost, f->card, dc, n, (uint32_t*)dout); break;
    case 2: hipLaunchKernelGGL(k_gather<uint16_t>, blocks_for((size_t)n), 256, 0, st, (const uint16_t*)f->data, f->plane_stride, ghost, f->card, dc, n, (uint16_t*)dout); break;
    default: hipLaunchKernelGGL(k_gather<uint8_t>, blocks_for((size_t)n), 256, 0, st, (const uint8_t*)f->data, f->plane_stride, ghost, f->card, dc, n, (uint8_t*)dout); break;
  }
  XLB_HIP(hipGetLastError());
  XLB_HIP(hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, st));
  XLB_HIP(hipStreamSynchronize(st));
  return 0;
}

int xlbhip_comm_stats(xlbhip_ctx* c, double* halo_wait_ms, int64_t* halo_waits, int reset) {
  XLB_REQUIRE(c, "ctx is null");
  for (int i = 0; i < xlbhip_ctx::WAIT_RING; ++i)
    if (int rc = harvest_wait(c, i)) return rc;
  if (halo_wait_ms) *halo_wait_ms = c->halo_wait_ms;
  if (halo_waits) *halo_waits = c->halo_waits;
  if (reset) {
    c->halo_wait_ms = 0.0;
    c->halo_waits = 0;
  }
  return 0;
}

int xlbhip_halo_exchange(xlbhip_ctx* c, int lattice, xlbhip_field* f) {
  XLB_REQUIRE(c && f, "null argument");
  XLB_REQUIRE(f->halo >= 1, "field has no ghost planes");
  XLB_REQUIRE(f->card == lattice_q(lattice), "field cardinality does not match the lattice");
  return halo_exchange_on(c, lattice, f, c->stream, 1);
}

int xlbhip_halo_exchange_wide(xlbhip_ctx* c, int lattice, xlbhip_field* f) {
  XLB_REQUIRE(c && f, "null argument");
  XLB_REQUIRE(f->halo >= 2, "field has fewer than two ghost planes per side");
  XLB_REQUIRE(f->card == lattice_q(lattice), "field cardinality does not match the lattice");
  return halo_exchange_on(c, lattice, f, c->stream, 2);
}

}  // extern "C"
