// The stepper's profile tables: per-cell prescribed values of Zou-He / Regularized BCs built with a profile, and the per-timestep
// wall velocities of HalfwayBounceBackBC / HybridBC with profile(cells, timestep).  The layout arithmetic is prof_table.hpp's, the
// ring's bookkeeping prof_ring.hpp's; this owner keeps the memory, the events and the copies.
#pragma once
#include <array>
#include <cstring>
#include <map>
#include <vector>

#include "api_internal.hpp"
#include "prof_ring.hpp"
#include "prof_table.hpp"

namespace xlb {

// Host map (storage cell -> 3 values) and its sorted device image.  The cells of time-dependent walls are entries of the same
// table, declared once (td_cells, in declaration order; td_pos = their rows in the sorted table).  Every timestep gets a full image
// of the table in one slot of a device ring (prof_ring.hpp keeps the books).  Images are staged through pinned host rows (one per
// slot, static entries written once), each guarded by the event of its last copy.  A stepper without time-dependent BCs has no
// ring and keeps its single table.
struct ProfileTables {
  xlbhip_ctx* ctx = nullptr;
  int cdt = 0;  // compute dtype of the values
  std::map<uint32_t, std::array<double, 3>> host;
  DeviceBuf keys;  // uint32 [n]
  DeviceBuf vals;  // compute dtype [n][3]
  int n = 0;
  std::vector<uint32_t> td_cells;
  std::vector<int> td_pos;
  bool td_contiguous = false;
  std::array<uint8_t, 256> td_bc{};  // bc ids with time-dependent cells
  std::vector<char> image;           // host copy of the table (compute dtype): the static entries of every image
  ProfRing book;
  DeviceBuf ring;  // [slots][n][3] compute dtype
  PinnedBuf pin;   // same layout
  std::vector<hipEvent_t> ev;
  std::vector<uint8_t> pin_ready;  // pinned row holds the static entries

  bool has_td() const { return !td_cells.empty(); }
  size_t image_bytes() const { return (size_t)n * 3 * (cdt == XLBHIP_F32 ? 4 : 8); }
  int slot_count() const { return has_td() ? prof_ring_slot_count(image_bytes()) : 0; }

  // the table the launches of timestep t read: the single table, or t's slot of the ring (nullptr: t is not staged)
  const void* table_at(int64_t t) const {
    if (!has_td()) return vals.get();
    const int k = book.find(t);
    return k < 0 ? nullptr : ring.get<char>() + (size_t)k * image_bytes();
  }
  // a time-dependent wall: the wall velocities of timestep t.  Any other BC: the single table (a kernel that evaluates one BC reads
  // entries of its cells only, and every staged image carries the same static entries), whatever is staged.
  const void* table_for(int bc_id, int64_t t) const { return td_bc[(size_t)bc_id] ? table_at(t) : vals.get(); }

  // the tables of the timesteps t0 .. t0 + count - 1 are all resident: checked before anything of a call is enqueued
  int require_staged(int64_t t0, int64_t count) const {
    if (!has_td()) return 0;
    for (int64_t k = 0; k < count; ++k)
      XLB_REQUIRE(table_at(t0 + k), "the time-dependent wall velocities of timestep %lld are not staged (xlbhip_stepper_stage_bc_profiles)",
                  (long long)(t0 + k));
    return 0;
  }

  // frees the ring (the stream must be drained: copies may still read the pinned rows)
  void release() {
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    (void)ring.reset();
    (void)pin.reset();
    ev.clear();
    pin_ready.clear();
    book.reset(0);
  }

  int add_static(int64_t count, const uint32_t* cells, const double* values) {
    for (int64_t i = 0; i < count; ++i) host[cells[i]] = {values[3 * i], values[3 * i + 1], values[3 * i + 2]};
    return rebuild();
  }

  int declare_time_dependent(int bc_id, int64_t count, const uint32_t* cells) {
    for (int64_t i = 0; i < count; ++i)
      XLB_REQUIRE(host.find(cells[i]) == host.end(), "cell %u has a profile table entry already", cells[i]);
    for (int64_t i = 0; i < count; ++i) {
      host[cells[i]] = {0.0, 0.0, 0.0};  // (placeholder: every image carries this timestep's value)
      td_cells.push_back(cells[i]);
    }
    if (count > 0) td_bc[(size_t)bc_id] = 1;
    return rebuild();
  }

  // the sorted device image of the merged table, its host copy and the rows of the time-dependent cells in it; drops the ring (its
  // images have the old layout).  Drains the stream first.
  int rebuild() {
    XLB_HIP(hipStreamSynchronize(ctx->stream));
    const ProfLayout lay = prof_table_layout(host, td_cells);
    n = (int)lay.keys.size();
    if (int rc = upload_keys(lay.keys, keys)) return rc;
    if (int rc = upload_values(cdt, lay.values, vals)) return rc;
    if (td_cells.empty() && !ring) return 0;
    image = compute_image(cdt, lay.values);
    td_pos = lay.td_pos;
    td_contiguous = lay.contiguous;
    release();
    return 0;
  }

  // the images of the timesteps t_first .. t_first + n_steps - 1 (values[n_steps][td_cells][3]) into the next slots of the ring
  int stage(int64_t t_first, int64_t n_steps, const double* values) {
    if (int rc = ensure_ring()) return rc;
    XLB_REQUIRE(n_steps <= book.slots(), "%lld tables staged at once, the ring holds %d (xlbhip_stepper_profile_slots)", (long long)n_steps,
                book.slots());
    const size_t img = image_bytes(), nt = td_cells.size();
    char* rows = pin.get<char>();
    int64_t r = 0;  // the image of timestep t_first + r goes next
    for (const ProfRing::Run run : book.take((int)n_steps)) {
      const int64_t r_first = r;
      for (int k = run.first; k < run.first + run.len; ++k, ++r) {
        XLB_HIP(hipEventSynchronize(ev[(size_t)k]));  // the previous copy out of this pinned row (not the kernels)
        char* row = rows + (size_t)k * img;
        if (!pin_ready[(size_t)k]) {
          std::memcpy(row, image.data(), img);
          pin_ready[(size_t)k] = 1;
        }
        by_compute(cdt, [&](auto T) {
          prof_fill_row(reinterpret_cast<decltype(T)*>(row), values + (size_t)r * nt * 3, td_pos, td_contiguous);
          return 0;
        });
      }
      // one copy per run of consecutive slots, on the compute stream: it lands after every kernel enqueued so far (those that still
      // read an older image of these slots) and before every launch that looks these timesteps up.  A slot counts as resident only
      // once its copy is enqueued; if that fails, nothing of the run is claimed.
      const size_t off = (size_t)run.first * img;
      XLB_HIP(hipMemcpyAsync(ring.get<char>() + off, rows + off, (size_t)run.len * img, hipMemcpyHostToDevice, ctx->stream));
      for (int k = run.first; k < run.first + run.len; ++k) {
        if (hipError_t e = hipEventRecord(ev[(size_t)k], ctx->stream); e != hipSuccess) {
          (void)hipStreamSynchronize(ctx->stream);  // (no copy out of a pinned row may stay in flight behind a stale event)
          XLB_FAIL("hipEventRecord: %s", hipGetErrorString(e));
        }
      }
      book.mark_resident(run, t_first + r_first);
    }
    return 0;
  }

 private:
  int ensure_ring() {
    if (ring) return 0;
    const int slots = slot_count();
    const size_t bytes = (size_t)slots * image_bytes();
    XLB_HIP(ring.alloc(bytes));
    if (hipError_t e = pin.alloc(bytes); e != hipSuccess) {
      release();
      XLB_FAIL("hipHostMalloc(%zu bytes) for the profile ring failed: %s", bytes, hipGetErrorString(e));
    }
    book.reset(slots);
    ev.assign((size_t)slots, nullptr);
    pin_ready.assign((size_t)slots, 0);
    for (int k = 0; k < slots; ++k) {
      if (hipError_t e = hipEventCreateWithFlags(&ev[(size_t)k], hipEventDisableTiming); e != hipSuccess) {
        ev.resize((size_t)k);
        release();
        XLB_FAIL("hipEventCreate: %s", hipGetErrorString(e));
      }
      XLB_HIP(hipEventRecord(ev[(size_t)k], ctx->stream));  // (every row starts out "copied")
    }
    return 0;
  }
};

}  // namespace xlb
