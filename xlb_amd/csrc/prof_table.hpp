// Layout of the profile table (profile_tables.hpp) and the fill of one of its per-timestep images: the merged, sorted table, the
// rows of the time-dependent cells in it, and the write of a timestep's wall velocities into those rows.  Host arithmetic only —
// no HIP type or call, so that tests/test_prof_table.py compiles it for the CPU; the device buffers and the copies are the owner's.
#pragma once
#include <algorithm>
#include <array>
#include <cstddef>
#include <cstdint>
#include <map>
#include <vector>

namespace xlb {

// a host table (storage cell -> N values, the first `width` of them used) as sorted keys and [n][width] values: std::map iterates
// in key order
template <class V, size_t N>
void sorted_table(const std::map<uint32_t, std::array<V, N>>& table, size_t width, std::vector<uint32_t>& keys, std::vector<V>& values) {
  keys.clear();
  values.clear();
  keys.reserve(table.size());
  values.reserve(table.size() * width);
  for (const auto& kv : table) {
    keys.push_back(kv.first);
    values.insert(values.end(), kv.second.begin(), kv.second.begin() + width);
  }
}

struct ProfLayout {
  std::vector<uint32_t> keys;  // sorted storage cells
  std::vector<double> values;  // [n][3]
  std::vector<int> td_pos;     // the row of every time-dependent cell, in declaration order
  bool contiguous = false;     // td_pos[i] == td_pos[0] + i: those rows are one block of the table
};

// `entries`: every cell of the table, the time-dependent ones (td_cells, in declaration order) with placeholder values
inline ProfLayout prof_table_layout(const std::map<uint32_t, std::array<double, 3>>& entries, const std::vector<uint32_t>& td_cells) {
  ProfLayout out;
  sorted_table(entries, 3, out.keys, out.values);
  out.td_pos.resize(td_cells.size());
  for (size_t i = 0; i < td_cells.size(); ++i)
    out.td_pos[i] = (int)(std::lower_bound(out.keys.begin(), out.keys.end(), td_cells[i]) - out.keys.begin());
  out.contiguous = true;
  for (size_t i = 0; i < out.td_pos.size(); ++i) out.contiguous = out.contiguous && out.td_pos[i] == out.td_pos[0] + (int)i;
  return out;
}

// values[nt][3] of one timestep (nt = td_pos.size(), declaration order) into the image row `row` ([n][3] of T); the other rows keep
// their contents.  contiguous (one time-dependent BC, or several whose cells are not interleaved with others): one block copy.
template <class T>
void prof_fill_row(T* row, const double* values, const std::vector<int>& td_pos, bool contiguous) {
  const size_t nt = td_pos.size();
  if (nt == 0) return;
  if (contiguous) {
    std::transform(values, values + 3 * nt, row + (size_t)td_pos[0] * 3, [](double v) { return (T)v; });
  } else {
    for (size_t i = 0; i < nt; ++i)
      for (int a = 0; a < 3; ++a) row[(size_t)td_pos[i] * 3 + a] = (T)values[i * 3 + a];
  }
}

}  // namespace xlb
