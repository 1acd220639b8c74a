// CPU driver of tests/test_prof_table.py: the layout of the profile table and the fill of one image row (xlb_amd/csrc/prof_table.hpp)
// for the commands read from stdin, one answer line each.
//   static KEY A B C   -> a static entry (written again: the later values); "ok"
//   td KEY             -> a time-dependent cell with placeholder values, in declaration order; "ok"
//   layout             -> "keys K K ... | td_pos P P ... | contiguous 0/1"
//   values             -> the table's values [n][3] as doubles
//   fill TYPE PATH V.. -> the image of the table in TYPE (f32 / f64) with the timestep's values V.. ([nt][3]) written by PATH: auto
//                         (the layout's contiguous flag), block or cells (forced); every element as the hex of its bytes
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "prof_table.hpp"

template <class T>
static void fill(const xlb::ProfLayout& lay, const std::vector<double>& v, bool contiguous) {
  std::vector<T> row(lay.values.begin(), lay.values.end());  // (the static entries, as the owner's host image holds them)
  xlb::prof_fill_row(row.data(), v.data(), lay.td_pos, contiguous);
  const char* sep = "";
  for (const T& x : row) {
    std::printf("%s", sep);
    for (size_t b = 0; b < sizeof(T); ++b) std::printf("%02x", reinterpret_cast<const unsigned char*>(&x)[b]);
    sep = " ";
  }
  std::printf("\n");
}

int main() {
  std::map<uint32_t, std::array<double, 3>> entries;
  std::vector<uint32_t> td_cells;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what;
    in >> what;
    if (what == "static") {
      uint32_t key = 0;
      double a = 0, b = 0, c = 0;
      in >> key >> a >> b >> c;
      entries[key] = {a, b, c};
      std::printf("ok\n");
    } else if (what == "td") {
      uint32_t key = 0;
      in >> key;
      entries[key] = {0.0, 0.0, 0.0};
      td_cells.push_back(key);
      std::printf("ok\n");
    } else if (what == "layout") {
      const xlb::ProfLayout lay = xlb::prof_table_layout(entries, td_cells);
      std::printf("keys");
      for (uint32_t k : lay.keys) std::printf(" %u", k);
      std::printf(" | td_pos");
      for (int p : lay.td_pos) std::printf(" %d", p);
      std::printf(" | contiguous %d\n", lay.contiguous ? 1 : 0);
    } else if (what == "values") {
      const xlb::ProfLayout lay = xlb::prof_table_layout(entries, td_cells);
      const char* sep = "";
      for (double v : lay.values) {
        std::printf("%s%.17g", sep, v);
        sep = " ";
      }
      std::printf("\n");
    } else if (what == "fill") {
      std::string type, path;
      in >> type >> path;
      std::vector<double> v;
      for (double x; in >> x;) v.push_back(x);
      const xlb::ProfLayout lay = xlb::prof_table_layout(entries, td_cells);
      if (v.size() != 3 * lay.td_pos.size() || (path == "block" && !lay.contiguous)) {
        std::printf("bad fill\n");
        continue;
      }
      const bool contiguous = path == "auto" ? lay.contiguous : path == "block";
      if (type == "f32")
        fill<float>(lay, v, contiguous);
      else
        fill<double>(lay, v, contiguous);
    }
  }
  return 0;
}
